"""Drop-in host side of the associative VAE: the reference's Python surface over libavae.

Mirrors the reference's vae_assoc.py: class ``AssocVariationalAutoEncoder`` (:20-463) with
``partial_fit / evaluate_cost / transform / generate / reconstruct / save_model / restore_model``
and the module function ``train`` (:498-583), same argument names, defaults and error behaviour.
Everything numerical happens in hand-written gfx950 kernels behind the C ABI of
include/avae.h; PyTorch-ROCm tensors only hold device memory.  There is no CPU path.

The class is spread over three modules.  This one holds what mirrors the reference: the constructor's host code
(``build_config``, ``initial_params``, ``create_replica``), the class with its training, evaluation, parameter and checkpoint
methods and the model's own forward-only calls (scoring, log-likelihood, ``complete``, ``impute``), ``train``, and the plumbing
every method goes through: ``_call`` (one checked library call on the model's handle and stream), ``_out``, ``_like_input``,
``_encode`` / ``_decode`` / ``_fused_decode``.  The two families the reference's class does not have are mixins it inherits:
``_latent_api.LatentAPI`` (DESIGN.md sections 18-22) and ``_pen_api.PenAPI`` (sections 23-30).  The checks are one validator per
entry point in ``_args``, over the array marshalling of ``_marshal``; their names are imported here and stay part of this
module's surface.

Deliberate, documented differences from the reference:
  * ``transfer_fct`` is a name ('relu', 'softplus', ...) or any callable whose ``__name__`` is
    one (``tf.nn.relu`` would qualify); the reference passes TF callables (:26,:502).
  * weights are drawn with NumPy (TF's RNG stream is not reproducible); same distribution as
    ``xavier_init`` (:11-18), biases zero.
  * ``partial_fit`` / ``evaluate_cost`` / ``reconstruct`` accept an optional explicit ``eps``
    (the reference draws it inside the graph, :90); ``None`` uses the in-kernel Philox stream.
  * network dicts may carry an extra key ``n_hidden`` (list) for more than two hidden layers.
  * ``hidden_conv=True`` (conv encoder :169-210 / deconv decoder :249-291, deconv.py) is built for what
    the reference's branch can express: a binary 28x28 modality (n_input = 784).
"""
import contextlib
import ctypes as C
import datetime
import os
import time

import numpy as np
import torch

from . import _capi
from ._args import (SEARCH_STATE_KEYS, _is_pair, _same_joints, agg_args, canvas_args, chain_matrices, draw_args,  # noqa: F401
                    embed_args, impute_args, latent_prior_args, latent_score_args, latent_stats_args, lognormal_augment_args,
                    lognormal_eval_args, lognormal_fit_args, lognormal_sample_options, motion_eval_args,
                    motion_fit_args, motion_fk_args, motion_ik_args, motion_matrices, motion_moments_args, motion_pose_args,
                    predict_motion_args, prior_arrays, refine_motion_args, refine_pen_path_args, render_args, search_args,
                    strokes_to_motion_args, topk_args, writing_cost_args,      # (the validators are part of this module's surface)
                    letter_thumbnail_args, occlude_quadrant, THUMBNAIL_CAMERA, THUMBNAIL_CANVAS,
                    check_solver, motion_track_args, track_rows_per_call, TRACK_FACTOR, TRACK_LAM_MAX, TRACK_LAM_MIN,
                    ADAM_STATE_KEYS, DESCENT_STATE_KEYS, adam_options, cost_weights, descend_motion_args, descent_state,
                    motion_eval_vjp_args, motion_fk_vjp_args, render_vjp_args, rows_adam_args,
                    chain_bodies, motion_dynamics_args, motion_effort_args)
from ._marshal import (as_index, corruption_fields, ema_fields, ema_kwargs, grad_clip_fields, grad_clip_kwargs, dev_array, dev_block3, dev_dense, dev_dense3, dev_flags, dev_inputs, dev_modalities, dev_row_args,  # noqa: F401
                       ld_of, ptr, schedule_kwargs, schedule_struct, to_device32)
from ._marshal import cyclical, exponential_decay, linear_warmup  # noqa: F401  (schedule helpers, part of this module's surface)
from ._latent_api import LatentAPI
from ._pen_api import PenAPI
from ._pen_api import (descend_motion, motion_eval_vjp, motion_fk_vjp, render_strokes_vjp, rows_adam,  # noqa: F401
                       writing_cost_grad)      # (functions of a model: DESIGN.md section 31)
from ._pen_api import motion_dynamics, motion_effort  # noqa: F401  (functions of a model: DESIGN.md section 32)
from .motion import MotionBasis  # noqa: F401
from .parallel import GradSync, dp_bucket_schedule, dp_train_step_bucketed

_ARCH_KEYS = ("scope", "hidden_conv", "n_hidden_recog_1", "n_hidden_recog_2",
              "n_hidden_gener_1", "n_hidden_gener_2", "n_input", "n_z")


def xavier_init(fan_in, fan_out, constant=1, rng=None):
    """Xavier initialisation of network weights (reference vae_assoc.py:11-18), as float32 NumPy."""
    low = -constant * np.sqrt(6.0 / (fan_in + fan_out))
    high = constant * np.sqrt(6.0 / (fan_in + fan_out))
    rng = np.random if rng is None else rng
    return rng.uniform(low, high, size=(fan_in, fan_out)).astype(np.float32)


def _act_name(transfer_fct):
    if transfer_fct is None:
        return "identity"
    name = transfer_fct if isinstance(transfer_fct, str) else getattr(transfer_fct, "__name__", str(transfer_fct))
    name = name.lower()
    if name not in _capi.ACT_IDS:
        raise ValueError("unsupported transfer_fct %r (supported: %s)" % (transfer_fct, sorted(_capi.ACT_IDS)))
    return name


def hidden_sizes(na):
    """Encoder widths of one modality.  The MLP decoder reuses them: the reference sizes its
    generator from n_hidden_recog_* and ignores n_hidden_gener_* (vae_assoc.py:257,280,293,299)."""
    if na.get("n_hidden") is not None:
        return [int(h) for h in na["n_hidden"]]
    return [int(na["n_hidden_recog_1"]), int(na["n_hidden_recog_2"])]


def layer_shapes(na):
    """Flat-parameter layout of one modality in the reference's variable-creation order
    (vae_assoc.py:185-215,257-300; conv branch :174-210,:251-300): [(name, shape), ...]."""
    if na.get("hidden_conv"):
        r1, r2 = int(na["n_hidden_recog_1"]), int(na["n_hidden_recog_2"])
        g1, g2 = int(na["n_hidden_gener_1"]), int(na["n_hidden_gener_2"])
        n_in, n_z = int(na["n_input"]), int(na["n_z"])
        shapes = [("enc_C1", (5, 5, 1, r1)), ("enc_C2", (5, 5, r1, 2 * r1)), ("enc_C3", (5, 5, 2 * r1, r2)),
                  ("enc_Wmu", (9 * r2, n_z)), ("enc_bmu", (n_z,)), ("enc_Wsig", (9 * r2, n_z)), ("enc_bsig", (n_z,))]
        for i, (k, co, ci) in enumerate(((3, g1, n_z), (5, g1 // 2, g1), (5, g2, g1 // 2), (5, 1, g2))):
            shapes += [("dec_T%d_W" % (i + 1), (k, k, co, ci)), ("dec_T%d_b" % (i + 1), (co,))]
        return shapes + [("dec_Wout", (n_in, n_in)), ("dec_bout", (n_in,))]
    hs = hidden_sizes(na)
    n_in, n_z = int(na["n_input"]), int(na["n_z"])
    shapes, prev = [], n_in
    for i, h in enumerate(hs):
        shapes += [("enc_W%d" % (i + 1), (prev, h)), ("enc_b%d" % (i + 1), (h,))]
        prev = h
    shapes += [("enc_Wmu", (prev, n_z)), ("enc_bmu", (n_z,)), ("enc_Wsig", (prev, n_z)), ("enc_bsig", (n_z,))]
    prev = n_z
    for i, h in enumerate(hs):
        shapes += [("dec_W%d" % (i + 1), (prev, h)), ("dec_b%d" % (i + 1), (h,))]
        prev = h
    shapes += [("dec_Wout", (prev, n_in)), ("dec_bout", (n_in,))]
    return shapes


def build_config(network_architectures, binary, weights, transfer_fct, assoc_lambda, learning_rate, batch_size, compute_dtype,
                 seed, use_graph, comm, comm_buckets, wire_dtype, placement):
    """The constructor's arguments -> (``_capi.Config``, binary list, weights list, activation name, comm): every field but the
    workspace and the collective's, after every check of the constructor in the constructor's order.  ``placement()`` ->
    (device index, world, rank) is called where the constructor opens the device and the process group, between the
    architecture checks and the collective's, so an input with several faults raises the same one first.  Pure host code:
    needs neither a GPU nor libavae.so."""
    n_mod = len(network_architectures)
    # check if binary data (vae_assoc.py:31-35)
    if type(binary) is list:
        assert len(binary) == n_mod
    else:
        binary = [binary] * n_mod
    if type(weights) is list:              # :37-41
        assert len(weights) == n_mod
    else:
        weights = [weights] * n_mod
    act = _act_name(transfer_fct)
    batch_size = int(batch_size)
    n_z = int(network_architectures[0]["n_z"])       # :89
    if n_mod > _capi.AVAE_MAX_MODALITIES:
        raise ValueError("at most %d modalities" % _capi.AVAE_MAX_MODALITIES)
    for na in network_architectures:
        if int(na["n_z"]) != n_z:
            raise ValueError("all modalities must share n_z (the reference builds one eps of modality 0's n_z, :89-91)")
        if na.get("hidden_conv") and int(na["n_input"]) != 784:
            raise ValueError("hidden_conv=True needs n_input = 784: the reference's branch is hard-wired to 28x28 images")
    if compute_dtype not in _capi.DTYPE_IDS:
        raise ValueError("compute_dtype must be 'bf16' or 'fp32'")
    device_index, world, rank = placement()
    if comm not in (None, "library", "torch", "ipc"):
        raise ValueError("comm must be None, 'library', 'ipc' or 'torch'")
    if comm is None:
        comm = "torch"
    if comm_buckets not in (1, 2):
        raise ValueError("comm_buckets must be 1 or 2")
    if wire_dtype not in _capi.DTYPE_IDS:
        raise ValueError("wire_dtype must be 'fp32' or 'bf16'")

    cfg = _capi.Config()
    cfg.abi_version = _capi.AVAE_ABI_VERSION
    cfg.n_modalities = n_mod
    for m, na in enumerate(network_architectures):
        hs = hidden_sizes(na)
        if len(hs) > _capi.AVAE_MAX_HIDDEN:
            raise ValueError("at most %d hidden layers" % _capi.AVAE_MAX_HIDDEN)
        cfg.mod[m].n_input = int(na["n_input"])
        cfg.mod[m].n_hidden_layers = len(hs)
        for k, hsz in enumerate(hs):
            cfg.mod[m].n_hidden[k] = hsz
        cfg.mod[m].binary = 1 if binary[m] else 0
        cfg.mod[m].weight = float(weights[m])
        cfg.mod[m].hidden_conv = 1 if na.get("hidden_conv") else 0
        if na.get("hidden_conv"):
            if not binary[m]:
                raise ValueError("hidden_conv=True needs a binary modality (the reference's non-binary conv decoder "
                                 "is shape-broken, vae_assoc.py:299)")
            cfg.mod[m].n_hidden_layers = 2
            cfg.mod[m].n_hidden[0], cfg.mod[m].n_hidden[1] = int(na["n_hidden_recog_1"]), int(na["n_hidden_recog_2"])
            cfg.mod[m].conv_gener[0], cfg.mod[m].conv_gener[1] = int(na["n_hidden_gener_1"]), int(na["n_hidden_gener_2"])
    cfg.n_z = n_z
    cfg.batch_size = batch_size
    cfg.batch_global = batch_size * world
    cfg.row_offset = rank * batch_size
    cfg.activation = _capi.ACT_IDS[act]
    cfg.compute_dtype = _capi.DTYPE_IDS[compute_dtype]
    cfg.device = device_index
    cfg.use_graph = 1 if use_graph else 0
    cfg.assoc_lambda = float(assoc_lambda)
    cfg.learning_rate = float(learning_rate)
    cfg.beta1 = cfg.beta2 = cfg.adam_eps = 0.0          # -> TF-1 AdamOptimizer defaults
    cfg.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    cfg.comm_buckets = comm_buckets
    cfg.wire_dtype = _capi.DTYPE_IDS[wire_dtype]
    return cfg, binary, weights, act, comm


def initial_params(network_architectures, seed):
    """The initial flat parameter vector: xavier-uniform weights, zero biases (vae_assoc.py:185-215,257-300), drawn with NumPy
    from ``seed`` in ``layer_shapes``' order.  Pure host code."""
    rng = np.random.RandomState(int(seed) & 0x7FFFFFFF)
    flat = []
    for na in network_architectures:
        for name, shp in layer_shapes(na):
            if len(shp) == 2:
                flat.append(xavier_init(shp[0], shp[1], rng=rng).reshape(-1))
            elif len(shp) == 4 and name.startswith("enc_C"):
                # weight_variable (vae_assoc.py:471-473): truncated_normal(stddev=0.1)
                w = rng.standard_normal(shp)
                while np.any(np.abs(w) > 2):
                    bad = np.abs(w) > 2
                    w[bad] = rng.standard_normal(int(bad.sum()))
                flat.append((0.1 * w).astype(np.float32).reshape(-1))
            elif len(shp) == 4:
                # deconv.py:83-84: xavier over (out_depth*k*k, in_depth*k*k)
                kk = shp[0] * shp[1]
                lim = np.sqrt(6.0 / (shp[2] * kk + shp[3] * kk))
                flat.append(rng.uniform(-lim, lim, size=shp).astype(np.float32).reshape(-1))
            else:
                flat.append(np.zeros(shp, dtype=np.float32))
    return np.concatenate(flat)


def create_replica(L, cfg, sync, comm, device, agree_dev):
    """Workspace + ``avae_create`` with the collective ``comm`` brought up -> (handle, comm in use, workspace tensor, buckets).

    Every step that needs the other ranks is agreed between them (``sync.sum_scalar``), in one fixed order on every rank: the
    RCCL probe, the ncclUniqueId broadcast, the verdict on ``avae_create``, the hipIpc handle all-gather, the verdict on the
    attach.  A collective that did not come up on every rank is dropped by all of them for 'torch'."""
    world = sync.world_size if sync else 1
    rank = sync.rank if sync else 0
    if comm == "library" and world > 1:
        # ncclCommInitRank below is collective: a rank that cannot even load RCCL would leave the others waiting inside it.  Every
        # rank therefore probes the loader first (drawing an id is the cheapest call that needs it) and the ranks agree: all, or
        # the torch.distributed collective on the same buckets for everybody.
        probe = (C.c_uint8 * 128)()
        ok = 1.0 if L.avae_comm_unique_id(probe) == 0 else 0.0
        if sync.sum_scalar(ok, agree_dev) < world:
            if rank == 0:
                print("[vae_assoc_amd] RCCL cannot be loaded on every rank: gradient all-reduce through torch.distributed")
            comm = "torch"
    if comm == "library":
        # bootstrap only: rank 0 draws the ncclUniqueId, torch.distributed hands it round; the communicator itself is the library's
        idb = (C.c_uint8 * 128)()
        if rank == 0:
            _capi.check(None, L.avae_comm_unique_id(idb), "avae_comm_unique_id")
        raw = sync.broadcast_bytes(bytes(idb), 128, device=agree_dev) if sync is not None else bytes(idb)
        cfg.use_comm, cfg.world_size, cfg.rank = _capi.COMM_RCCL, world, rank
        for i in range(128):
            cfg.nccl_id[i] = raw[i]
    elif comm == "ipc":
        cfg.use_comm, cfg.world_size, cfg.rank = _capi.COMM_IPC, world, rank
    # data-parallel buckets (host-only query): [[(offset, count), ...] per bucket]
    nb, nr = C.c_int32(0), (C.c_int32 * 2)()
    offs, cnts = (C.c_int64 * 2)(), (C.c_int64 * 2)()
    _capi.check(None, L.avae_dp_plan(C.byref(cfg), C.byref(nb), nr, offs, cnts), "avae_dp_plan")
    buckets = [[(int(offs[b]), int(cnts[b]))] for b in range(nb.value)]      # ONE contiguous range per bucket
    nbytes = C.c_size_t(0)
    _capi.check(None, L.avae_workspace_bytes(C.byref(cfg), C.byref(nbytes)), "avae_workspace_bytes")
    # PyTorch is the device allocator: one uint8 tensor holds the whole replica state
    ws = torch.empty(nbytes.value + 256, dtype=torch.uint8, device=device)
    base = ws.data_ptr()
    cfg.workspace = base + (-base) % 256
    cfg.workspace_bytes = nbytes.value
    h = C.c_void_p()
    torch.cuda.synchronize(device)
    rc = L.avae_create(C.byref(cfg), C.byref(h))
    if comm in ("library", "ipc") and world > 1:
        # Bring-up is agreed between the ranks at every collective step: a communicator / exchange that came up on some ranks
        # only is of no use to any.  RCCL: ncclCommInitRank ran inside avae_create.  IPC: every rank that created its replica
        # exports its exchange block, the handles go round (all_gather), every rank maps its peers' blocks.
        ok = 1.0 if rc == 0 else 0.0
        all_ok = sync.sum_scalar(ok, agree_dev) >= world
        if all_ok and comm == "ipc":
            mine = (C.c_uint8 * _capi.AVAE_IPC_HANDLE_BYTES)()
            ok = 1.0 if L.avae_comm_ipc_handle(h, mine) == 0 else 0.0
            blob = sync.all_gather_bytes(bytes(mine), _capi.AVAE_IPC_HANDLE_BYTES, device=agree_dev)
            if ok:
                buf = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
                ok = 1.0 if L.avae_comm_ipc_attach(h, buf) == 0 else 0.0
                if not ok:
                    print("[vae_assoc_amd] rank %d: %s" % (rank, L.avae_last_error(h).decode("utf-8", "replace")))
            all_ok = sync.sum_scalar(ok, agree_dev) >= world
        if not all_ok:
            if rc == 0:
                L.avae_destroy(h)
            if rank == 0:
                print("[vae_assoc_amd] the library's %s collective did not come up on every rank: gradient all-reduce "
                      "through torch.distributed" % ("RCCL" if comm == "library" else "hipIpc"))
            comm = "torch"
            cfg.use_comm = _capi.COMM_NONE
            h = C.c_void_p()
            rc = L.avae_create(C.byref(cfg), C.byref(h))
    _capi.check(None, rc, "avae_create")
    return h, comm, ws, buckets


class AssocVariationalAutoEncoder(LatentAPI, PenAPI):
    """Associative VAE over M sensory modalities, trained on one MI355X (or one per rank).

    Same constructor signature as the reference (vae_assoc.py:26-27); keyword-only extras:
      compute_dtype  'bf16' (default: bf16 MFMA operands, fp32 accumulate/loss/Adam) or 'fp32'
      device         torch device / ordinal (default: current CUDA(HIP) device)
      seed           seeds the NumPy weight draw and the in-kernel eps generator
      use_graph      replay the step as a captured hipGraph
      data_parallel  True -> one replica per torch.distributed rank, sample-sharded batch, the gradient SUM-all-reduced per
                     step in two buckets (decoder side first, overlapping the encoder's backward pass), Adam per bucket
      comm           who runs that collective:
                       'ipc'     libavae's own one-shot all-reduce over hipIpc peers (push reduce-scatter + push all-gather, every
                                 xGMI link at once; torch.distributed only hands the exchange-block handles round);
                       'library' libavae's RCCL communicator (ncclAllReduce on the library's comm stream; torch.distributed only
                                 hands the ncclUniqueId round);
                       'torch'   torch.distributed.all_reduce over the same buckets, the host stepping the pipeline.
                     None = 'torch' for world > 1 (the path every multi-rank parity test runs; pass 'ipc' / 'library' to opt in --
                     bench.py does), 'torch' for one rank.  comm='library' / 'ipc' without data_parallel builds a one-rank
                     communicator (tests)
      comm_buckets   2 (default): decoder-side bucket first, its all-reduce beside the encoder's backward pass; 1: ONE all-reduce of
                     the whole gradient buffer after the backward pass (north_star's literal design)
      wire_dtype     'fp32' (default) or 'bf16': element type of the gradient on the wire (the cost always travels as fp32)
      corruption     None, or a dict of ``set_corruption``'s arguments (``drop``, ``noise``, ``drop_value``): denoising training,
                     every training step corrupts the encoder's copy of the batch on the device while the losses keep the clean one
      grad_clip      None, a number (``max_norm``) or a dict of ``set_grad_clip``'s arguments (``max_norm``, ``skip_nonfinite``):
                     clip every step's gradient by its global norm and / or skip a step whose gradient is not finite
      schedule       None, or a dict of ``set_schedule``'s arguments (``kl``, ``assoc``, ``lr``; steps): KL warm-up, association
                     ramp and learning-rate decay, evaluated on the device per training step
      ema            None, a number (``decay``) or a dict of ``set_ema``'s arguments (``decay``, ``warmup``): keep an exponential
                     average of the parameters on the device; ``averaged()`` runs inference and evaluation on it
    """

    def __init__(self, network_architectures, binary=True, transfer_fct="softplus", weights=1.0,
                 assoc_lambda=1.0, learning_rate=0.001, batch_size=100, *, compute_dtype="bf16",
                 device=None, seed=0, use_graph=True, data_parallel=False, process_group=None, comm=None,
                 comm_buckets=2, wire_dtype="fp32", corruption=None, grad_clip=None, schedule=None, ema=None):
        clip_kw = grad_clip_kwargs(grad_clip)        # (a bad value raises before anything is built)
        ema_kw = ema_kwargs(ema)
        if schedule is not None and isinstance(schedule, dict) and schedule.get("unit", "step") != "step":
            raise ValueError("schedule: the constructor counts in steps (unit='step'); train() converts unit='epoch'")
        sched_kw = schedule_kwargs(schedule)
        def placement():
            if not torch.cuda.is_available():
                raise RuntimeError("vae_assoc_amd needs a HIP device (MI355X / gfx950); there is no CPU fallback")
            dev = torch.cuda.current_device() if device is None else device
            self.device = torch.device("cuda", dev if isinstance(dev, int) else torch.device(dev).index or 0)
            self._sync = GradSync(process_group) if data_parallel else None
            return (self.device.index,) + ((self._sync.world_size, self._sync.rank) if self._sync else (1, 0))

        cfg, self.binary, self.weights, _act, comm = build_config(
            network_architectures, binary, weights, transfer_fct, assoc_lambda, learning_rate, batch_size, compute_dtype, seed,
            use_graph, comm, comm_buckets, wire_dtype, placement)
        self.network_architectures = network_architectures
        self.assoc_lambda = assoc_lambda
        self.transfer_fct = transfer_fct
        self.learning_rate = learning_rate
        self.compute_dtype = compute_dtype
        self.batch_size, self.n_z = cfg.batch_size, cfg.n_z
        self._widths = tuple(int(na["n_input"]) for na in network_architectures)
        L = _capi.lib()
        self._agree_dev = self.device if (self._sync is not None and self._sync.backend == "nccl") else "cpu"
        h, self._comm, self._ws, self._buckets = create_replica(L, cfg, self._sync, comm, self.device, self._agree_dev)
        self._comm_lib = self._comm in ("library", "ipc")
        self._cfg = cfg
        self._h = h
        self._L = L
        n = C.c_size_t(0)
        self._call_host("avae_param_count", C.byref(n))
        self.n_params = n.value
        gp, gn = C.c_void_p(), C.c_size_t(0)
        self._call_host("avae_grad_buffer", C.byref(gp), C.byref(gn))
        goff = gp.value - self._ws.data_ptr()
        self._grad_view = self._ws[goff:goff + 4 * gn.value].view(torch.float32)
        self.set_params(initial_params(network_architectures, seed))
        if corruption is not None:
            self.set_corruption(**corruption)
        if clip_kw:
            self.set_grad_clip(**clip_kw)
        if sched_kw:
            self.set_schedule(**sched_kw)
        if ema_kw:
            self.set_ema(**ema_kw)

    # ------------------------------------------------------------------ plumbing
    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._L.avae_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _call(self, name, *args):
        """Library entry point ``name`` on the model's handle, ``args`` and the current stream; a failure raises under ``name``"""
        _capi.check(self._h, getattr(self._L, name)(self._h, *args, self._stream()), name)

    def _call_host(self, name, *args):
        """``_call`` for the entry points that take no stream"""
        _capi.check(self._h, getattr(self._L, name)(self._h, *args), name)

    def _out(self, shape, dtype=torch.float32):
        """uninitialised tensor on the model's device: an output of a library call"""
        return torch.empty(shape, dtype=dtype, device=self.device)

    @staticmethod
    def _ptrs(ts):
        """per-modality tensors (None -> NULL) -> the ``void*[M]`` the library takes"""
        return (C.c_void_p * len(ts))(*[ptr(t) for t in ts])

    @staticmethod
    def _like_input(was_np):
        """NumPy in gives NumPy out, device tensors in give device tensors out -> the conversion of one output (None stays None)"""
        return (lambda a: None if a is None else a.cpu().numpy()) if was_np else (lambda a: a)

    def _twin(self, name, head, p, tail):
        """Call entry point ``name`` or, with presence bytes ``p``, its ``_masked`` twin, which takes them after (x, ld): the one
        place where a call picks between the two."""
        if p is not None:
            name, head = name + "_masked", head + (p.data_ptr(),)
        self._call(name, *head, *tail)

    def _batch_args(self, X, eps, n_steps=1, present=None, inputs=None):
        """Arguments of the training / eval entry points -> (device tensors, ptrs, lds, eps tensor or None, presence or None,
        explicit inputs (tensors, ptrs, lds) or None).
        ``present`` (the masked entry points): [batch_size * n_steps, M] -> uint8 device tensor, and ``X[m] = None`` -> a NULL
        source (modality m absent on every row).  ``inputs`` (the ``_in`` entry points): the encoder's rows, a list like ``X``
        with None where a modality has no explicit input."""
        # the reference's eps has static shape (batch_size, n_z): every path through z needs exactly batch_size rows (vae_assoc.py:90)
        rows = self.batch_size * n_steps
        what = "batch_size x n_steps" if n_steps > 1 else "batch_size"
        p = None
        if present is None:
            assert len(X) == len(self._widths)
        else:
            world = self._sync.world_size if self._sync is not None else 1
            if world > 1:
                raise RuntimeError("present= (partially paired batches) runs on one replica; this model is data parallel over %d ranks" % world)
            p = dev_flags(present, len(self._widths), self.device, rows, what)
        ts, _, _, ptrs, lds = dev_modalities(X, self._widths, self.device, rows, what, allow_none=p is not None)
        ins = None if inputs is None else dev_inputs(inputs, ts, self._widths, self.device, rows, what)
        return ts, ptrs, lds, dev_dense(eps, self.n_z, self.device, rows, what), p, ins

    def _call_in(self, name, head, ins, p, tail):
        """Entry point ``name`` with explicit encoder inputs ``ins`` (and optional presence bytes ``p``): the ``_in`` calls take
        both after (x, ld)."""
        self._call(name, *head, ins[1], ins[2], ptr(p), *tail)

    def _train(self, X, n_steps, eps, present, return_cost, one_step=False, inputs=None):
        ts, ptrs, lds, e, p, ins = self._batch_args(X, eps, n_steps, present, inputs)
        cost = C.c_float(0.0)
        tail = (ptr(e), C.byref(cost) if return_cost else None)
        if ins is not None:
            self._call_in("avae_train_steps_in", (n_steps, ptrs, lds), ins, p, tail)
        elif one_step and p is None:    # (library-owned collective: avae_train_step runs the bucketed pipeline itself)
            self._twin("avae_train_step", (ptrs, lds), None, tail)
        else:
            self._twin("avae_train_steps", (n_steps, ptrs, lds), p, tail)
        return cost.value if return_cost else None

    def get_params(self):
        out = np.empty(self.n_params, dtype=np.float32)
        self._call_host("avae_get_params", out.ctypes.data_as(C.c_void_p))
        return out

    def set_params(self, flat):
        flat = np.ascontiguousarray(flat, dtype=np.float32).reshape(-1)
        if flat.size != self.n_params:
            raise ValueError("expected %d parameters, got %d" % (self.n_params, flat.size))
        self._call_host("avae_set_params", flat.ctypes.data_as(C.c_void_p))

    def get_grads(self):
        out = np.empty(self.n_params, dtype=np.float32)
        self._call_host("avae_get_grads", out.ctypes.data_as(C.c_void_p))
        return out

    def get_opt_state(self):
        m = np.empty(self.n_params, dtype=np.float32)
        v = np.empty(self.n_params, dtype=np.float32)
        step = C.c_int64(0)
        self._call_host("avae_get_opt_state", m.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p), C.byref(step))
        return m, v, step.value

    def set_opt_state(self, m=None, v=None, step=0):
        """Restores the Adam moments (flat float32 arrays in ``get_params``' order; None leaves one as it is) and the step
        counter -- what ``get_opt_state`` returns.  The counter keys the eps / corruption streams and the training schedules."""
        def arr(a):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.float32).ravel()
            if a.size != self.n_params:
                raise ValueError("expected %d values, got %d" % (self.n_params, a.size))
            return a
        m, v = arr(m), arr(v)
        self._call_host("avae_set_opt_state", None if m is None else m.ctypes.data_as(C.c_void_p),
                        None if v is None else v.ctypes.data_as(C.c_void_p), C.c_int64(int(step)))

    def cost_history(self, n):
        out = np.empty(n, dtype=np.float32)
        last = C.c_int64(0)
        self._call_host("avae_cost_history", n, out.ctypes.data_as(C.c_void_p), C.byref(last))
        return out

    def set_corruption(self, drop=0.0, noise=0.0, drop_value=0.0):
        """Denoising training (avae_set_corruption in include/avae.h): from now on every training step
        feeds the encoders a corrupted copy of the batch, drawn on the device, while the reconstruction terms are charged against
        the clean batch.  Per element, independently: with probability ``drop`` it is replaced by ``drop_value`` (0 = erased
        ink), else N(0, ``noise``^2) is added.  Each argument is a scalar (every modality) or a list with one value per modality;
        ``set_corruption(None)`` (or all zeros) turns it off.  A modality given through ``inputs=`` is not corrupted.

        Evaluation stays clean: ``evaluate_cost``, the early-stop validation cost of ``train`` and every inference call ignore
        the setting.  The draw is keyed by (seed, step, global row, modality, column): under data parallelism every rank must be
        built with the same ``seed``, as for eps.  The setting is not saved by ``save_model``."""
        p, s, d = corruption_fields(drop, noise, drop_value, len(self._widths))
        c = _capi.Corruption()
        for m in range(len(self._widths)):
            c.drop_prob[m], c.noise_std[m], c.drop_value[m] = p[m], s[m], d[m]
        self._call_host("avae_set_corruption", C.byref(c))

    def set_grad_clip(self, max_norm=0.0, skip_nonfinite=False):
        """Global-norm gradient clipping and non-finite step skipping (avae_set_grad_clip in include/avae.h, DESIGN.md section
        15) -- where a TF-1 caller of the reference wrote ``tf.clip_by_global_norm`` in front of the optimiser.  From now on every
        training step measures the norm of its whole gradient (the all-reduced one under data parallelism) and Adam consumes
        ``g * max_norm / norm`` whenever ``norm > max_norm``; ``get_grads`` keeps returning the raw gradient.
        ``max_norm=float('inf')`` only monitors (``grad_norm_history``), ``max_norm=0`` does not clip.  ``skip_nonfinite=True``:
        a step whose gradient holds a NaN or Inf (or whose sum of squares overflows fp32) leaves the parameters and the Adam
        moments untouched; it still counts as a step (step counter, eps keys, cost history).  Both off (the default) is the
        step as it was.  The call synchronises the device; the setting is not saved by ``save_model``."""
        mx, skip = grad_clip_fields(max_norm, skip_nonfinite)
        self._call_host("avae_set_grad_clip", C.c_float(mx), skip)

    def grad_norm_history(self, n):
        """-> (norms, last_step, n_skipped): the raw (unclipped) gradient norms of the most recent ``n`` steps as a float32
        array, oldest first; the step number of the last one; the number of steps skipped since the model was built.  ``n`` may
        not exceed the number of steps trained since ``set_grad_clip`` switched the feature on (nor the history's 4096)."""
        out = np.empty(n, dtype=np.float32)
        last, skipped = C.c_int64(0), C.c_int64(0)
        self._call_host("avae_grad_norm_history", n, out.ctypes.data_as(C.c_void_p), C.byref(last), C.byref(skipped))
        return out, last.value, skipped.value

    def set_schedule(self, kl=None, assoc=None, lr=None):
        """Training schedules, evaluated on the device for every step (avae_set_schedule in include/avae.h, DESIGN.md section
        16): ``kl`` multiplies the KL terms (beta warm-up / cyclical annealing), ``assoc`` multiplies ``assoc_lambda`` (ramping the
        association penalty in), ``lr`` multiplies ``learning_rate`` (where a TF-1 caller wrote ``tf.train.exponential_decay``).
        Each is None (off: multiplier 1), a number (constant multiplier), ``dict(knots=[(step, value), ...], period=None)`` --
        linear between up to 8 knots, constant outside, repeating every ``period`` steps when given -- or ``dict(decay_rate=,
        decay_steps=, staircase=False)``; ``linear_warmup``, ``cyclical`` and ``exponential_decay`` build such dicts.  ``step``
        counts the steps taken before the one in question (0 for the first step of a fresh model); the value depends on the step
        counter alone, so a restored model (``restore_model``, ``set_opt_state``) continues its schedule.

        The KL multiplier is a multiplication: 0 does not hide a non-finite KL term.  Evaluation never reads a schedule:
        ``evaluate_cost``, the early-stop cost of ``train`` and every inference call use the configured objective.
        ``set_schedule()`` switches everything off.  The call synchronises the device; the setting is not saved by ``save_model``."""
        sc = [schedule_struct(v, name) for v, name in ((kl, "kl"), (assoc, "assoc"), (lr, "lr"))]
        self._call_host("avae_set_schedule", *[None if x is None else C.byref(x) for x in sc])

    def hyper_history(self, n):
        """-> (values, last_step): ``values[i] = (kl_t, lambda_t, lr_eff_t)`` of the most recent ``n`` steps as a float32 array
        [n, 3], oldest first -- the KL multiplier, the scheduled ``assoc_lambda`` and the scheduled ``learning_rate`` the step
        used -- and the step number of the last one.  ``n`` may not exceed the number of steps trained since ``set_schedule``
        switched a schedule on (nor the history's 4096)."""
        out = np.empty((n, 3), dtype=np.float32)
        last = C.c_int64(0)
        self._call_host("avae_hyper_history", n, out.ctypes.data_as(C.c_void_p), C.byref(last))
        return out, last.value

    def set_ema(self, decay, warmup=False):
        """Parameter averaging (avae_set_ema in include/avae.h) -- where a TF-1 caller of the reference
        wrote ``tf.train.ExponentialMovingAverage(decay).apply(...)`` behind the optimiser.  From now on every training step also
        moves an average of the parameters, kept on the device, towards the step's new parameters:
        ``avg -= (avg - theta) * (1 - d_t)`` with ``d_t = decay``, or with ``warmup=True`` TF's ``num_updates`` form
        ``d_t = min(decay, (1 + t) / (10 + t))``, t the step's number.  Switching it on starts the average at the current
        parameters; training itself (parameters, moments, costs) is bit for bit what it is without it.  A step skipped by
        ``skip_nonfinite`` leaves the average alone.  ``decay`` None or 0 switches it off; changing ``decay`` / ``warmup`` while
        it is on keeps the average.  ``averaged()`` / ``use_averaged`` run inference on the average, ``get_ema_params`` reads it,
        ``save_model`` stores it (with ``decay`` and ``warmup``) and ``restore_model`` brings it back.  The call synchronises
        the device."""
        d, w = ema_fields(decay, warmup)
        self._call_host("avae_set_ema", C.c_float(d), w)

    def get_ema_params(self):
        """The averaged parameters, flat float32 in ``get_params``' order (an error while averaging is off)."""
        out = np.empty(self.n_params, dtype=np.float32)
        self._call_host("avae_get_ema", out.ctypes.data_as(C.c_void_p))
        return out

    def set_ema_params(self, flat):
        """Replaces the averaged parameters (flat, ``get_params``' order; an error while averaging is off)."""
        flat = np.ascontiguousarray(flat, dtype=np.float32).reshape(-1)
        if flat.size != self.n_params:
            raise ValueError("expected %d parameters, got %d" % (self.n_params, flat.size))
        self._call_host("avae_set_ema_params", flat.ctypes.data_as(C.c_void_p))

    def use_averaged(self, on=True):
        """``on``: every inference call (``transform``, ``generate``, ``reconstruct``, ``score_samples``, ``log_likelihood``,
        ``complete``, ``impute``, their masked twins) and ``evaluate_cost`` run on the averaged parameters from now on, and every
        training call raises; ``on=False`` switches back to the live ones.  One launch that rebuilds the compute-dtype weights;
        ``get_params`` keeps returning the live parameters.  ``set_params`` and ``restore_model`` leave the model on the live
        parameters."""
        self._call_host("avae_use_averaged", 1 if on else 0)

    @contextlib.contextmanager
    def averaged(self):
        """``with model.averaged(): ...`` -- ``use_averaged(True)`` for the block, always switched back after it."""
        self.use_averaged(True)
        try:
            yield self
        finally:
            self.use_averaged(False)

    def synchronize(self):
        self._call_host("avae_synchronize")

    # ------------------------------------------------------------------ data-parallel seam (parallel.py protocol)
    def _backward(self, X, eps=None, inputs=None):
        """local forward + backward + every weight gradient: the gradient buffer (and the local cost in its last float) is complete"""
        self._stage(X, eps, inputs=inputs)
        for b in range(len(self._buckets)):
            self._backward_bucket(b)

    def _apply(self, want_cost=True):
        cost = None
        for b in range(len(self._buckets)):
            cost = self._apply_bucket(b, want_cost and b == len(self._buckets) - 1)
        return cost

    def _grad_tensor(self):
        return self._grad_view

    # bucketed seam (parallel.dp_train_step_bucketed): stage -> per bucket backward / all-reduce -> per bucket Adam
    def _stage(self, X, eps=None, n_steps=1, inputs=None):
        ts, ptrs, lds, e, _, ins = self._batch_args(X, eps, n_steps, inputs=inputs)
        self._stage_run(n_steps, ts, lds, e, ins, 0)
        self._staged_j = 0

    def _stage_run(self, n, ts, lds, e, ins, i0):
        """stages batches [i0, i0 + n) of the marshalled run (``avae_stage_batches``, or its ``_in`` twin with explicit inputs)"""
        B = self.batch_size
        at = lambda t: None if t is None else t.data_ptr() + i0 * B * t.stride(0) * 4
        p_i = (C.c_void_p * len(ts))(*[at(t) for t in ts])
        e_i = (e.data_ptr() + i0 * B * self.n_z * 4) if e is not None else None
        if ins is None:
            self._call("avae_stage_batches", n, p_i, lds, e_i)
        else:
            in_i = (C.c_void_p * len(ts))(*[at(t) for t in ins[0]])
            self._call("avae_stage_batches_in", n, p_i, lds, in_i, ins[2], e_i)

    def _backward_bucket(self, b):
        self._call("avae_dp_backward", self._staged_j, b)

    def _apply_bucket(self, b, want_cost=True):
        cost = C.c_float(0.0)
        self._call("avae_dp_apply", b, C.byref(cost) if want_cost else None)
        return cost.value if want_cost else None

    # ------------------------------------------------------------------ reference surface
    def partial_fit(self, X, eps=None, return_cost=True, present=None, inputs=None):
        """Train model based on mini-batch of input data.  Return cost of mini-batch.
        (reference vae_assoc.py:378-386).  ``return_cost=False`` skips the host synchronise;
        the cost stays retrievable through ``cost_history``.

        ``present`` (optional, one replica): [batch_size, M] presence flags, nonzero = row n has modality m.  The step then charges
        every row only with the terms of the modalities it has (include/avae.h; the divisor stays batch_size),
        and ``X[m]`` may be None for a modality absent from the whole batch.

        ``inputs`` (optional): explicit encoder inputs, a list like ``X`` whose entries may be None -- the encoder of modality m
        reads ``inputs[m]`` while every loss term is charged against ``X[m]`` (denoising training with corruption of the caller's
        own; ``set_corruption`` draws one on the device instead).  Column views of one wide matrix work without a copy, as for
        ``X``."""
        if present is None and self._sync is not None and self._sync.world_size > 1 and not self._comm_lib:
            # host-owned collective (torch.distributed) over the library's buckets
            cost = dp_train_step_bucketed(self, self._sync, self._buckets, X, eps, inputs)
            return cost if return_cost else None
        return self._train(X, 1, eps, present, return_cost, one_step=True, inputs=inputs)

    def partial_fit_steps(self, X, n_steps, eps=None, return_cost=True, present=None, inputs=None):
        """``n_steps`` successive ``partial_fit`` calls in one submission: step i trains on rows
        [i*batch_size, (i+1)*batch_size) of every X[m] (and of ``eps``) -- what the reference's inner
        loop does with ``DataSet.next_batch``'s consecutive slices (vae_assoc.py:541-550).  Returns the
        last step's cost; every step's cost is in ``cost_history``.  ``present``: [n_steps * batch_size, M]
        presence flags, ``inputs``: explicit encoder inputs of the same rows, both as in ``partial_fit``."""
        n_steps = int(n_steps)
        if present is not None or self._sync is None or self._sync.world_size == 1 or self._comm_lib:
            return self._train(X, n_steps, eps, present, return_cost, inputs=inputs)
        # host-owned collective: the batches are staged 16 at a time, every step runs the bucketed schedule
        ts, ptrs, lds, e, _, ins = self._batch_args(X, eps, n_steps, inputs=inputs)
        cost = None
        for i0 in range(0, n_steps, 16):
            n = min(16, n_steps - i0)
            self._stage_run(n, ts, lds, e, ins, i0)
            for j in range(n):
                self._staged_j = j
                cost = dp_bucket_schedule(self, self._sync, self._buckets, return_cost and i0 + j == n_steps - 1)
        return cost

    def evaluate_cost(self, X, eps=None, present=None, inputs=None):
        """reference vae_assoc.py:388-391 (forward + loss with a fresh eps, no update).  ``present``: [batch_size, M] presence
        flags, as in ``partial_fit`` (one replica).  ``inputs``: explicit encoder inputs as in ``partial_fit`` -- the objective on
        given corrupted inputs; a corruption set with ``set_corruption`` never applies here."""
        ts, ptrs, lds, e, p, ins = self._batch_args(X, eps, present=present, inputs=inputs)
        cost = C.c_float(0.0)
        if ins is not None:
            self._call_in("avae_eval_cost_in", (ptrs, lds), ins, p, (ptr(e), C.byref(cost)))
        else:
            self._twin("avae_eval_cost", (ptrs, lds), p, (ptr(e), C.byref(cost)))
        c = cost.value
        if self._sync is not None and self._sync.world_size > 1:        # (never with ``present``: that runs on one replica)
            c = self._sync.sum_scalar(c, self.device)
        return c

    def _encode(self, m, x, want_logvar=False):
        t, was_np = dev_array(x, self._widths[m], self.device)
        rows = t.shape[0]
        mu = self._out((rows, self.n_z))
        lv = torch.empty_like(mu) if want_logvar else None
        if rows:
            self._call("avae_encode", m, t.data_ptr(), ld_of(t), rows, mu.data_ptr(), ptr(lv))
        conv = self._like_input(was_np)
        return (conv(mu), conv(lv)) if want_logvar else conv(mu)

    def transform(self, X, sens_idx=None):
        """Transform data by mapping it into the latent space (posterior means only).
        ``sens_idx`` is None (X = list over modalities) or an integer (X = one array)
        (reference vae_assoc.py:393-403)."""
        if sens_idx is None:
            return [self._encode(m, x) for m, x in enumerate(X)]
        assert sens_idx < len(self.network_architectures)
        return self._encode(sens_idx, X)

    def generate(self, z_mu=None):
        """Generate data by sampling from latent space: decoder only, z fed directly; returns the
        list of per-modality decoder means.  ``None`` draws z from the prior with NumPy's global
        RNG, batch_size rows (reference vae_assoc.py:405-419)."""
        if z_mu is None:
            z_mu = np.random.normal(size=(self.batch_size, self.n_z))
        z = dev_dense(z_mu, self.n_z, self.device)
        rows = z.shape[0]
        outs = [self._out((rows, cols)) for cols in self._widths]
        if rows:       # every modality's decoder in one submission (avae_generate: one graph replay for 1-64 rows)
            self._call("avae_generate", z.data_ptr(), rows, self._ptrs(outs))
        conv = self._like_input(not torch.is_tensor(z_mu))
        return [conv(o) for o in outs]

    def reconstruct(self, X, eps=None):
        """Use VAE to reconstruct given data: encode -> sample z -> decode, per modality with its
        own eps draw as each sess.run of the reference makes one (vae_assoc.py:421-425).
        ``eps`` may be a list with one [rows, n_z] array per modality."""
        outs = []
        for m, (x, cols) in enumerate(zip(X, self._widths)):
            t, was_np = dev_array(x, cols, self.device)
            rows = t.shape[0]
            e = dev_dense(eps[m], self.n_z, self.device) if eps is not None else None
            assert e is None or e.shape[0] == rows
            o = self._out((rows, cols))
            if rows:
                self._call("avae_reconstruct", m, t.data_ptr(), ld_of(t), ptr(e), rows, o.data_ptr())
            outs.append(self._like_input(was_np)(o))
        return outs

    def score_samples(self, X, eps=None, cross_modal=False):
        """Per-row terms of the training cost, for any number of rows (forward only; avae_score in include/avae.h).

        ``X`` is a list over modalities with equal row counts; ``eps`` an [N, n_z] array shared by every modality, or None for
        a fresh internal draw.  Returns a dict of ``cost [N]``, ``recon [N, M]``, ``latent [N, M]``, ``assoc [N, P]`` (pairs
        (i<j) in lexicographic order) and, with ``cross_modal=True``, ``cross [N, M, M]``: cross[n, s, d] is the reconstruction
        loss of modality d decoded from the posterior mean of modality s.  NumPy in gives NumPy out, device tensors in give
        device tensors out."""
        return self._score(X, None, eps, cross_modal)

    def score_samples_masked(self, X, present, eps=None, cross_modal=False):
        """``score_samples`` for partially paired rows (avae_score_masked in include/avae.h).

        ``present`` is an [N, M] bool / integer array or tensor (any device), nonzero = row n has modality m; ``X[m] = None`` marks
        a modality absent from every row.  Absent entries are never read: fill them with anything.  Returns ``score_samples``'
        dict: ``recon`` / ``latent`` hold 0 where the row lacks the modality, ``assoc`` 0 where it lacks either of the pair, ``cost``
        sums the terms the row has, and ``cross[n, s, d]`` is NaN where the row lacks s or d.  Every present entry except ``cost``
        is bitwise ``score_samples``' value for the same rows and eps."""
        return self._score(X, present, eps, cross_modal)

    def _score(self, X, present, eps, cross_modal):
        M = len(self.network_architectures)
        ts, rows, was_np, ptrs, lds, p = dev_row_args(X, self._widths, self.device, present)
        e = dev_dense(eps, self.n_z, self.device, rows)
        flags = _capi.SCORE_CROSS if cross_modal else 0
        k = C.c_int32(0)
        _capi.check(None, self._L.avae_score_width(C.byref(self._cfg), flags, C.byref(k)), "avae_score_width")
        out = self._out((rows, k.value))
        if rows:
            self._twin("avae_score", (ptrs, lds), p, (rows, ptr(e), flags, out.data_ptr()))
        out = self._like_input(was_np)(out)      # one [N, k] array: the entries below are views of it
        P = M * (M - 1) // 2
        res = {"cost": out[:, 0], "recon": out[:, 1:1 + M], "latent": out[:, 1 + M:1 + 2 * M],
               "assoc": out[:, 1 + 2 * M:1 + 2 * M + P]}
        if cross_modal:
            res["cross"] = out[:, 1 + 2 * M + P:].reshape(rows, M, M)
        return res

    def log_likelihood(self, X, n_samples=64, eps=None):
        """Importance-weighted (IWAE) estimates of held-out log-likelihoods with K = ``n_samples`` samples per proposal (forward
        only; avae_loglik in include/avae.h).

        ``X`` is a list over modalities with equal row counts; ``eps`` an [N, n_samples, n_z] array (sample k of row n is shared by
        every proposal), or None for a fresh internal draw.  The proposal of modality s is its encoder's posterior q_s(z | x_s);
        the reconstruction terms are score_samples' (Bernoulli with the 1e-3 inside the log, Gaussian 0.5 ||x - x_hat||^2 without
        the 2 pi constant; no modality weights, no assoc_lambda).  Returns a dict of natural-log estimates:
        ``marginal [N, M]`` (log p(x_m), proposal q_m), ``joint [N, M]`` (log p(x_1..x_M), proposal q_s) and ``conditional
        [N, M, M]``: conditional[n, s, d] estimates log p(x_d | x_s) = log E_{q_s}[p(x_d | z)], the diagonal included.  NumPy in
        gives NumPy out, device tensors in give device tensors out.  Under data parallelism each replica scores its own rows:
        there is no collective."""
        return self._loglik(X, None, n_samples, eps)

    def log_likelihood_masked(self, X, present, n_samples=64, eps=None):
        """``log_likelihood`` for partially paired rows (avae_loglik_masked in include/avae.h).

        ``present`` and ``X[m] = None`` as in ``score_samples_masked``.  Returns ``log_likelihood``'s dict: ``marginal[n, s]`` is
        NaN where row n lacks s, ``conditional[n, s, d]`` NaN where it lacks s or d, and ``joint[n, s]`` is the log-likelihood of
        the modalities the row has under proposal q_s (NaN where it lacks s).  A row with nothing present is all NaN."""
        return self._loglik(X, present, n_samples, eps)

    def _loglik(self, X, present, n_samples, eps):
        M = len(self.network_architectures)
        if isinstance(n_samples, bool) or not isinstance(n_samples, (int, np.integer)) or n_samples < 1:
            raise ValueError("n_samples must be an integer >= 1, got %r" % (n_samples,))
        K = int(n_samples)
        ts, rows, was_np, ptrs, lds, p = dev_row_args(X, self._widths, self.device, present)
        e = dev_dense3(eps, (rows, K, self.n_z), self.device)
        out = self._out((rows, 2 * M + M * M))
        if rows:
            self._twin("avae_loglik", (ptrs, lds), p, (rows, K, ptr(e), out.data_ptr()))
        out = self._like_input(was_np)(out)      # one [N, k] array: the entries below are views of it
        return {"marginal": out[:, :M], "joint": out[:, M:2 * M], "conditional": out[:, 2 * M:].reshape(rows, M, M)}

    def complete(self, X, observed=None, n_iters=50, lr=0.05, prior_weight=1.0, z0=None, init=None):
        """Gradient latent refinement for partially observed rows (avae_complete in include/avae.h): per
        row, the z that minimises ``J(z) = sum_m w_m recon_obs_m(x_m, dec_m(z), o_m) + prior_weight * 0.5 |z|^2`` is searched with
        ``n_iters`` steps of per-row Adam (step size ``lr``) through the decoders, the whole loop on the device, and every
        modality is decoded from the result.

        ``X`` is a list over modalities with equal row counts; ``X[m] = None`` means modality m is unobserved.  ``observed`` is
        None (everything given is observed) or a list over modalities of ``[N, n_input_m]`` bool / integer element masks, nonzero
        = observed, ``observed[m] = None`` = modality m fully observed.  Unobserved elements are never read: fill them with
        anything.  The start is ``z0`` (``[N, n_z]``) or, without it, the posterior mean of modality ``init`` (default: the first
        modality that is not None) encoded with its unobserved elements set to 0, as the reference encodes the blanked image
        (baxter_vae_assoc_writer.py:501-511).  ``n_iters = 0`` evaluates only.

        Returns a dict: ``z [N, n_z]``, ``x`` (list over modalities of ``[N, n_input_m]`` decoder outputs at ``z``, the unobserved
        parts and modalities included), ``objective [n_iters + 1, N]`` (J at the start and after every update) and ``grad0
        [N, n_z]`` (dJ/dz at the start).  NumPy in gives NumPy out, device tensors in give device tensors out."""
        widths = self._widths
        M = len(widths)
        if len(X) != M:
            raise ValueError("expected a list of %d modalities, got %d" % (M, len(X)))
        if observed is not None and len(observed) != M:
            raise ValueError("observed must be None or a list of %d element masks, got %d" % (M, len(observed)))
        if isinstance(n_iters, bool) or not isinstance(n_iters, (int, np.integer)) or n_iters < 0:
            raise ValueError("n_iters must be an integer >= 0, got %r" % (n_iters,))
        n_iters = int(n_iters)
        ts, rows, was_np, xp, lds = dev_modalities(X, widths, self.device, allow_none=True)
        if rows is None:
            raise ValueError("every modality is None: nothing is observed")
        obs = [None] * M
        for m, o in enumerate(() if observed is None else observed):
            if o is not None and ts[m] is not None:
                obs[m] = dev_flags(o, widths[m], self.device, rows, "as X[%d]" % m, "observed[%d]" % m)
        if z0 is None:
            init = next(m for m in range(M) if ts[m] is not None) if init is None else init
            if isinstance(init, bool) or not isinstance(init, (int, np.integer)) or not 0 <= init < M or ts[init] is None:
                raise ValueError("init must be the index of a modality that is not None, got %r" % (init,))
            xi = ts[init] if obs[init] is None else torch.where(obs[init] != 0, ts[init], torch.zeros_like(ts[init]))
            z = self._encode(init, xi).contiguous()
        else:
            z = dev_dense(z0, self.n_z, self.device, rows, name="z0")
        out_z, grad, obj = self._out((rows, self.n_z)), self._out((rows, self.n_z)), self._out((n_iters + 1, rows))
        outs = [self._out((rows, cols)) for cols in widths]
        if rows:
            self._call("avae_complete", xp, lds, self._ptrs(obs), z.data_ptr(), rows, n_iters, float(lr), float(prior_weight),
                       out_z.data_ptr(), obj.data_ptr(), grad.data_ptr(), self._ptrs(outs))
        conv = self._like_input(was_np)
        return {"z": conv(out_z), "x": [conv(o) for o in outs], "objective": conv(obj), "grad0": conv(grad)}

    def impute(self, X, present=None, n_samples=0, eps=None):
        """Predict every modality from the ones each row has (avae_impute in include/avae.h): the
        per-modality posteriors of the present modalities are fused into the Gaussian closest to all of them in the symmetric-KL
        sense the model is trained with (precision = mean of the precisions, precision-weighted mean), and every decoder runs on it.

        ``X`` is a list over modalities, ``X[m] = None`` a modality absent from every row; ``present`` is None (every given
        modality is present on every row) or an [N, M] bool / integer array or tensor as in ``score_samples_masked``.  The row
        count comes from ``present``, or else from the first modality that is not None.  Absent entries are never read.  A row
        with one modality gets exactly that modality's posterior, a row with none the prior (mu = logvar = 0).
        ``n_samples = 0`` decodes the fused mean once (``generate(mu)``); ``n_samples = K >= 1`` decodes K samples
        ``z_k = mu + exp(logvar / 2) eps_k`` and returns the per-element mean and population variance over them, without ever
        holding the ``N K n_input`` decoded values.  ``eps`` is an [N, K, n_z] array or None for a fresh internal draw (the draw
        counter is the one ``score_samples`` / ``log_likelihood`` advance).

        Returns a dict: ``mu [N, n_z]``, ``logvar [N, n_z]``, ``mean`` (list over modalities of ``[N, n_input_m]``, present
        modalities included: for them it is a reconstruction) and ``var`` (such a list, or None when ``n_samples == 0``).  NumPy
        in gives NumPy out, device tensors in give device tensors out."""
        widths = self._widths
        ts, rows, was_np, xp, lds, p, K, e = impute_args(X, present, n_samples, eps, widths, self.n_z, self.device)
        mu, lv = self._out((rows, self.n_z)), self._out((rows, self.n_z))
        mean = [self._out((rows, cols)) for cols in widths]
        var = [self._out((rows, cols)) for cols in widths] if K else None
        if rows:
            self._call("avae_impute", xp, lds, ptr(p), rows, K, ptr(e), mu.data_ptr(), lv.data_ptr(), self._ptrs(mean),
                       self._ptrs(var) if K else None)
        conv = self._like_input(was_np)
        return {"mu": conv(mu), "logvar": conv(lv), "mean": [conv(o) for o in mean],
                "var": [conv(o) for o in var] if K else None}

    def _fused_decode(self, xp, lds, p, rows, modality, want_mean):
        """avae_impute with no samples -> (mu, logvar, the decoded fused mean of ``modality`` or None)"""
        mu, lv = self._out((rows, self.n_z)), self._out((rows, self.n_z))
        mean = [None] * len(self._widths)
        if want_mean:
            mean[modality] = self._out((rows, self._widths[modality]))
        if rows:
            self._call("avae_impute", xp, lds, ptr(p), rows, 0, None, mu.data_ptr(), lv.data_ptr(), self._ptrs(mean), None)
        return mu, lv, mean[modality]

    def _decode(self, modality, z, out=None):
        """avae_decode on device tensors: latents ``z [rows, n_z]`` -> the parameters of ``modality`` (into ``out`` if given)"""
        if out is None:
            out = self._out((z.shape[0], self._widths[modality]))
        if z.shape[0]:
            self._call("avae_decode", modality, z.data_ptr(), z.shape[0], out.data_ptr())
        return out

    def save_model(self, fname=None):
        """reference vae_assoc.py:427-435 (default name: timestamp + batch size)."""
        if fname is None:
            ts = time.time()
            ckpt_fname = 'vae_assoc_' + datetime.datetime.fromtimestamp(ts).strftime('%Y_%m_%d_%H_%M_%S') \
                + '_batchsize_{}.ckpt'.format(self.batch_size)
        else:
            ckpt_fname = fname
        print('Saving model to {}...'.format(ckpt_fname))
        self._call_host("avae_save", os.fsencode(ckpt_fname))
        return

    def restore_model(self, folder=None, fname=None):
        """reference vae_assoc.py:437-463: newest-listed *.ckpt of ``folder`` ('output' by default)
        unless ``fname`` is given; every failure prints and returns, nothing raises."""
        model_folder = 'output' if folder is None else folder
        if os.path.isdir(model_folder) and os.path.exists(model_folder):
            if fname is None:
                files = [f for f in os.listdir(model_folder) if f.endswith('.ckpt')]
                if not files:
                    print('No valid model file.')
                    return
                model_file = files[-1]
            else:
                model_file = fname
            path = os.path.join(model_folder, model_file)
            if os.path.exists(path):
                print('Loading {}...'.format(path))
                rc = self._L.avae_load(self._h, os.fsencode(path))
                if rc != 0:
                    print('Invalid or non-exist model file. ({})'.format(self._L.avae_last_error(self._h).decode()))
            else:
                print('Invalid or non-exist model file.')
        else:
            print('Invalid or non-exist model folder.')
        return


def train(data_sets, network_architectures, binary=True, weights=1.0, assoc_lambda=1e-5, learning_rate=0.001,
          batch_size=100, training_epochs=10, display_step=5, early_stop=False, **model_kwargs):
    """Epoch/minibatch loop of the reference (vae_assoc.py:498-583): relu transfer (:502), column
    split of the [N, sum n_input] matrix (:510,:543), optional validation early stop (:520-537),
    ``avg_cost_hist`` = running within-epoch sum appended per batch (:576-577).

    Runs of consecutive ``next_batch`` slices (everything between two reshuffles) are handed over as one
    matrix and trained in one submission (``partial_fit_steps``); the matrix is split into modalities on
    the device by pointer offset + row stride (no per-modality copies); per-step costs are read back once
    per epoch from the device-side history, so the hot loop never synchronises.

    ``data_parallel=True`` (one process per GPU): ``batch_size`` is the per-rank batch; every rank walks the SAME
    data set in the SAME order in global batches of ``world * batch_size`` rows and trains on its own rows of each
    (see ``train_loop``), so the run equals the single-process run with ``batch_size * world``.

    ``corruption=dict(drop=..., noise=..., drop_value=...)`` (``set_corruption``'s arguments) trains with the denoising
    criterion: every training step corrupts the encoders' copy of its batch on the device, the losses keep the clean rows.  The
    validation cost of ``early_stop`` stays clean.  Under ``data_parallel`` every rank must pass the same ``seed``, as for eps.

    ``grad_clip=max_norm`` or ``grad_clip=dict(max_norm=..., skip_nonfinite=...)`` (``set_grad_clip``'s arguments) clips every
    step's gradient by its global norm and / or skips a step whose gradient is not finite.

    ``schedule=dict(kl=..., assoc=..., lr=..., unit='step')`` (``set_schedule``'s arguments) anneals the KL weight, ramps the
    association penalty and decays the learning rate on the device.  With ``unit='epoch'`` the knot steps, periods and
    ``decay_steps`` count epochs of this loop: they are multiplied by its ``total_batch = n_samples // (batch_size * world)``.
    The validation cost of ``early_stop`` is the configured objective, whatever the schedule.

    ``ema=decay`` or ``ema=dict(decay=..., warmup=True)`` (``set_ema``'s arguments) keeps an exponential average of the parameters
    on the device; use the returned model's ``averaged()`` for inference on it.  The validation cost of ``early_stop`` stays on
    the live parameters."""
    schedule = model_kwargs.pop("schedule", None)
    # (a bad value raises before anything is built; train_loop converts again with the world size the model ends up with)
    schedule_kwargs(schedule, steps_per_epoch=int(data_sets.train._data.shape[0] / batch_size))
    vae_assoc =AssocVariationalAutoEncoder(network_architectures, binary, transfer_fct="relu", weights=weights,
                                            assoc_lambda=assoc_lambda, learning_rate=learning_rate,
                                            batch_size=batch_size, **model_kwargs)
    return train_loop(vae_assoc, data_sets, network_architectures, batch_size, training_epochs, display_step, early_stop,
                      schedule=schedule)


def train_loop(vae_assoc, data_sets, network_architectures, batch_size, training_epochs=10, display_step=5,
               early_stop=False, sync=None, device=None, schedule=None):
    """The loop of ``train`` on an already built model (any object with ``partial_fit`` / ``evaluate_cost``, and optionally
    ``partial_fit_steps`` / ``cost_history``; the CPU tests drive it with an oracle-backed replica).

    Data parallelism (``sync`` = the model's ``GradSync``, world > 1): the reference's loop (vae_assoc.py:516-577) is kept, with
    the global batch ``B_g = world * batch_size`` in the place of ``batch_size``: ``next_batch(B_g)`` on every rank -- rank 0's
    NumPy seed is broadcast first, and a checksum of the training matrix is compared, so that all ranks shuffle alike --
    rank r trains on rows [r*batch_size, (r+1)*batch_size) of it, ``total_batch = n_samples // B_g`` and the (already
    all-reduced, global-batch) cost enters ``avg_cost`` with weight ``B_g / n_samples``.

    ``schedule`` (``train``'s keyword): handed to the model's ``set_schedule`` before the first step, a schedule in epochs
    converted to steps with this loop's ``total_batch``."""
    if sync is None:
        sync = getattr(vae_assoc, "_sync", None)
    world = sync.world_size if sync is not None else 1
    rank = sync.rank if sync is not None else 0
    n_samples = data_sets.train._data.shape[0]
    sens_indices = np.concatenate([[0], np.cumsum([na["n_input"] for na in network_architectures])])
    n_mod = len(network_architectures)
    avg_cost_hist = []
    valid_cost = None
    dev = device if device is not None else getattr(vae_assoc, "device", None)
    hist_cap = 4096
    batch_global = batch_size * world
    lo, hi = rank * batch_size, (rank + 1) * batch_size
    if schedule is not None:
        vae_assoc.set_schedule(**schedule_kwargs(schedule, steps_per_epoch=int(n_samples / batch_global)))
    # a training split that carries presence (dataset.DataSet(present=)): masked steps, and a masked validation cost
    masked = getattr(data_sets.train, "_present", None) is not None
    if masked and (world > 1 or getattr(vae_assoc, "_comm_lib", False)):
        raise RuntimeError("train() on a data set with presence (partially paired rows) runs on one replica; this model is "
                           "data parallel (%d ranks%s)" % (world, ", library-owned collective" if world == 1 else ""))
    if world > 1:
        boot_dev = getattr(vae_assoc, "_agree_dev", "cpu" if dev is None else dev)
        np.random.seed(sync.broadcast_int(int(np.random.randint(0, 2 ** 31 - 1)), device=boot_dev))
        # every rank must hold the SAME training matrix in the SAME order: rank 0's digest of ~256 sampled rows (content and
        # position both enter) goes round, every rank compares its own with it, and the verdicts are all-reduced so that either
        # every rank raises or none does (a rank that raised alone would leave the others waiting in the next collective)
        d = data_sets.train._data
        rows = d[:: max(1, n_samples // 256)]
        rows = rows.double().cpu().numpy() if torch.is_tensor(rows) else np.asarray(rows, dtype=np.float64)
        wts = np.cos(np.arange(rows.size, dtype=np.float64).reshape(rows.shape) * 0.7548776662466927)
        digest = np.array([n_samples, rows.shape[1], float((rows * wts).sum()), float(np.abs(rows).sum())], dtype=np.float64)
        ref = np.frombuffer(sync.broadcast_bytes(digest.tobytes(), digest.nbytes, device=boot_dev), dtype=np.float64)
        same = bool(np.all(np.abs(ref - digest) <= 1e-9 * np.maximum(1.0, np.abs(ref))))
        if not sync.all_agree(same, boot_dev):
            raise ValueError("data_parallel train(): the ranks hold different training matrices (or different orders of one); "
                             "build the data sets from the same array with the same NumPy seed on every rank")

    def seg(batch_xs):
        # host batches (reference DataSet) are uploaded once per step; a dataset.DeviceDataSet hands device rows
        if dev is None:
            t = np.asarray(batch_xs)
        else:
            t = batch_xs if torch.is_tensor(batch_xs) else torch.as_tensor(np.ascontiguousarray(batch_xs, dtype=np.float32))
            t = t.to(dev)
        return [t[:, sens_indices[k]:sens_indices[k + 1]] for k in range(n_mod)]

    def shard_run(batch_xs, n):
        """rows of this rank inside each of the n consecutive global batches, as one matrix of n*batch_size rows"""
        if world == 1:
            return batch_xs
        t = batch_xs.reshape(n, batch_global, batch_xs.shape[1])[:, lo:hi]
        return t.reshape(n * batch_size, batch_xs.shape[1])

    def pres(split):
        """presence rows of the slice the split handed out last; a split without presence (a fully paired validation set next
        to a partially paired training set) counts as all present"""
        p = split.last_present()
        if p is None:
            lo_, hi_ = split.last_rows()
            p = np.ones((hi_ - lo_, n_mod), dtype=np.uint8)
        return p

    multi = hasattr(vae_assoc, "partial_fit_steps") and hasattr(vae_assoc, "cost_history")
    for epoch in range(training_epochs):
        avg_cost = 0.
        total_batch = int(n_samples / batch_global)
        if early_stop:
            if epoch % early_stop == 0:
                curr_valid_cost = 0
                n_valid_batches = int(data_sets.validation._data.shape[0] / batch_global)
                for i in range(n_valid_batches):
                    batch_xs, _ = data_sets.validation.next_batch(batch_global)
                    if masked:
                        curr_valid_cost += vae_assoc.evaluate_cost(seg(batch_xs), present=pres(data_sets.validation)) / n_valid_batches
                        continue
                    curr_valid_cost += vae_assoc.evaluate_cost(seg(shard_run(batch_xs, 1))) / n_valid_batches
                print("Validation cost=", "{:.9f}".format(curr_valid_cost))
                if valid_cost is not None:
                    if curr_valid_cost > valid_cost:
                        print('Validation error increases. Early stop at epoch {} to prevent overfitting...'.format(epoch + 1))
                        break
                valid_cost = curr_valid_cost
        done = 0
        while done < total_batch:
            chunk = min(hist_cap, total_batch - done)
            got = 0
            costs = []
            while got < chunk:
                if multi and hasattr(data_sets.train, "next_batches"):     # a run of consecutive slices = one submission
                    batch_xs, _, n = data_sets.train.next_batches(batch_global, chunk - got)
                    if masked:
                        vae_assoc.partial_fit_steps(seg(batch_xs), n, return_cost=False, present=pres(data_sets.train))
                    else:
                        vae_assoc.partial_fit_steps(seg(shard_run(batch_xs, n)), n, return_cost=False)
                else:                                             # a reference-style DataSet object
                    batch_xs, _ = data_sets.train.next_batch(batch_global)
                    kw = {"return_cost": False} if multi else {}
                    if masked:
                        kw["present"] = pres(data_sets.train)
                    c = vae_assoc.partial_fit(seg(shard_run(batch_xs, 1)), **kw)
                    costs.append(c)
                    n = 1
                got += n
            for cost in (vae_assoc.cost_history(chunk) if multi else costs):
                avg_cost += float(cost) / n_samples * batch_global
                avg_cost_hist.append(avg_cost)
            done += chunk
        if epoch % display_step == 0:
            print("Epoch:", '%04d' % (epoch + 1), "cost=", "{:.9f}".format(avg_cost))
    return vae_assoc, avg_cost_hist
