"""Drop-in host side of the associative VAE: the reference's Python surface over libavae.

Mirrors /root/reference/vae_assoc.py: class ``AssocVariationalAutoEncoder`` (:20-463) with
``partial_fit / evaluate_cost / transform / generate / reconstruct / save_model / restore_model``
and the module function ``train`` (:498-583), same argument names, defaults and error behaviour.
Everything numerical happens in hand-written gfx950 kernels behind the C ABI of
include/avae.h; PyTorch-ROCm tensors only hold device memory.  There is no CPU path.

This module holds the constructor's host code (``build_config``, ``initial_params``, ``create_replica``), the class, whose
methods are library calls on checked arguments, and ``train``.  The checks are one validator per entry point in ``_args``,
over the array marshalling of ``_marshal``; their names are imported here and stay part of this module's surface.

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
                    check_solver, motion_track_args, track_rows_per_call, TRACK_FACTOR, TRACK_LAM_MAX, TRACK_LAM_MIN)
from ._marshal import (as_index, corruption_fields, ema_fields, ema_kwargs, grad_clip_fields, grad_clip_kwargs, dev_array, dev_block3, dev_dense, dev_dense3, dev_flags, dev_inputs, dev_modalities, dev_row_args,  # noqa: F401
                       ld_of, ptr, schedule_kwargs, schedule_struct, to_device32)
from ._marshal import cyclical, exponential_decay, linear_warmup  # noqa: F401  (schedule helpers, part of this module's surface)
from .motion import MotionBasis
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


class AssocVariationalAutoEncoder(object):
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
        _capi.check(h, L.avae_param_count(h, C.byref(n)), "avae_param_count")
        self.n_params = n.value
        gp, gn = C.c_void_p(), C.c_size_t(0)
        _capi.check(h, L.avae_grad_buffer(h, C.byref(gp), C.byref(gn)), "avae_grad_buffer")
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

    def _new(self, rows, cols):
        """uninitialised float32 [rows, cols] on the model's device: an output of a forward-only call"""
        return torch.empty((rows, cols), dtype=torch.float32, device=self.device)

    @staticmethod
    def _ptrs(ts):
        """per-modality tensors (None -> NULL) -> the ``void*[M]`` the library takes"""
        return (C.c_void_p * len(ts))(*[ptr(t) for t in ts])

    @staticmethod
    def _like_input(was_np):
        """NumPy in gives NumPy out, device tensors in give device tensors out -> the conversion of one output"""
        return (lambda a: a.cpu().numpy()) if was_np else (lambda a: a)

    def _twin(self, name, head, p, tail):
        """Call entry point ``name`` or, with presence bytes ``p``, its ``_masked`` twin, which takes them after (x, ld): the one
        place where a call picks between the two."""
        if p is not None:
            name, head = name + "_masked", head + (p.data_ptr(),)
        _capi.check(self._h, getattr(self._L, name)(self._h, *head, *tail, self._stream()), name)

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
        _capi.check(self._h, getattr(self._L, name)(self._h, *head, ins[1], ins[2], ptr(p), *tail, self._stream()), name)

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
        _capi.check(self._h, self._L.avae_get_params(self._h, out.ctypes.data_as(C.c_void_p)), "avae_get_params")
        return out

    def set_params(self, flat):
        flat = np.ascontiguousarray(flat, dtype=np.float32).reshape(-1)
        if flat.size != self.n_params:
            raise ValueError("expected %d parameters, got %d" % (self.n_params, flat.size))
        _capi.check(self._h, self._L.avae_set_params(self._h, flat.ctypes.data_as(C.c_void_p)), "avae_set_params")

    def get_grads(self):
        out = np.empty(self.n_params, dtype=np.float32)
        _capi.check(self._h, self._L.avae_get_grads(self._h, out.ctypes.data_as(C.c_void_p)), "avae_get_grads")
        return out

    def get_opt_state(self):
        m = np.empty(self.n_params, dtype=np.float32)
        v = np.empty(self.n_params, dtype=np.float32)
        step = C.c_int64(0)
        _capi.check(self._h, self._L.avae_get_opt_state(self._h, m.ctypes.data_as(C.c_void_p),
                                                        v.ctypes.data_as(C.c_void_p), C.byref(step)), "avae_get_opt_state")
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
        _capi.check(self._h, self._L.avae_set_opt_state(self._h, None if m is None else m.ctypes.data_as(C.c_void_p),
                                                        None if v is None else v.ctypes.data_as(C.c_void_p), C.c_int64(int(step))),
                    "avae_set_opt_state")

    def cost_history(self, n):
        out = np.empty(n, dtype=np.float32)
        last = C.c_int64(0)
        _capi.check(self._h, self._L.avae_cost_history(self._h, n, out.ctypes.data_as(C.c_void_p), C.byref(last)),
                    "avae_cost_history")
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
        _capi.check(self._h, self._L.avae_set_corruption(self._h, C.byref(c)), "avae_set_corruption")

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
        _capi.check(self._h, self._L.avae_set_grad_clip(self._h, C.c_float(mx), skip), "avae_set_grad_clip")

    def grad_norm_history(self, n):
        """-> (norms, last_step, n_skipped): the raw (unclipped) gradient norms of the most recent ``n`` steps as a float32
        array, oldest first; the step number of the last one; the number of steps skipped since the model was built.  ``n`` may
        not exceed the number of steps trained since ``set_grad_clip`` switched the feature on (nor the history's 4096)."""
        out = np.empty(n, dtype=np.float32)
        last, skipped = C.c_int64(0), C.c_int64(0)
        _capi.check(self._h, self._L.avae_grad_norm_history(self._h, n, out.ctypes.data_as(C.c_void_p), C.byref(last),
                                                            C.byref(skipped)), "avae_grad_norm_history")
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
        _capi.check(self._h, self._L.avae_set_schedule(self._h, *[None if x is None else C.byref(x) for x in sc]), "avae_set_schedule")

    def hyper_history(self, n):
        """-> (values, last_step): ``values[i] = (kl_t, lambda_t, lr_eff_t)`` of the most recent ``n`` steps as a float32 array
        [n, 3], oldest first -- the KL multiplier, the scheduled ``assoc_lambda`` and the scheduled ``learning_rate`` the step
        used -- and the step number of the last one.  ``n`` may not exceed the number of steps trained since ``set_schedule``
        switched a schedule on (nor the history's 4096)."""
        out = np.empty((n, 3), dtype=np.float32)
        last = C.c_int64(0)
        _capi.check(self._h, self._L.avae_hyper_history(self._h, n, out.ctypes.data_as(C.c_void_p), C.byref(last)), "avae_hyper_history")
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
        _capi.check(self._h, self._L.avae_set_ema(self._h, C.c_float(d), w), "avae_set_ema")

    def get_ema_params(self):
        """The averaged parameters, flat float32 in ``get_params``' order (an error while averaging is off)."""
        out = np.empty(self.n_params, dtype=np.float32)
        _capi.check(self._h, self._L.avae_get_ema(self._h, out.ctypes.data_as(C.c_void_p)), "avae_get_ema")
        return out

    def set_ema_params(self, flat):
        """Replaces the averaged parameters (flat, ``get_params``' order; an error while averaging is off)."""
        flat = np.ascontiguousarray(flat, dtype=np.float32).reshape(-1)
        if flat.size != self.n_params:
            raise ValueError("expected %d parameters, got %d" % (self.n_params, flat.size))
        _capi.check(self._h, self._L.avae_set_ema_params(self._h, flat.ctypes.data_as(C.c_void_p)), "avae_set_ema_params")

    def use_averaged(self, on=True):
        """``on``: every inference call (``transform``, ``generate``, ``reconstruct``, ``score_samples``, ``log_likelihood``,
        ``complete``, ``impute``, their masked twins) and ``evaluate_cost`` run on the averaged parameters from now on, and every
        training call raises; ``on=False`` switches back to the live ones.  One launch that rebuilds the compute-dtype weights;
        ``get_params`` keeps returning the live parameters.  ``set_params`` and ``restore_model`` leave the model on the live
        parameters."""
        _capi.check(self._h, self._L.avae_use_averaged(self._h, 1 if on else 0), "avae_use_averaged")

    @contextlib.contextmanager
    def averaged(self):
        """``with model.averaged(): ...`` -- ``use_averaged(True)`` for the block, always switched back after it."""
        self.use_averaged(True)
        try:
            yield self
        finally:
            self.use_averaged(False)

    def synchronize(self):
        _capi.check(self._h, self._L.avae_synchronize(self._h), "avae_synchronize")

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
            _capi.check(self._h, self._L.avae_stage_batches(self._h, n, p_i, lds, e_i, self._stream()), "avae_stage_batches")
        else:
            in_i = (C.c_void_p * len(ts))(*[at(t) for t in ins[0]])
            _capi.check(self._h, self._L.avae_stage_batches_in(self._h, n, p_i, lds, in_i, ins[2], e_i, self._stream()),
                        "avae_stage_batches_in")

    def _backward_bucket(self, b):
        _capi.check(self._h, self._L.avae_dp_backward(self._h, self._staged_j, b, self._stream()), "avae_dp_backward")

    def _apply_bucket(self, b, want_cost=True):
        cost = C.c_float(0.0)
        _capi.check(self._h, self._L.avae_dp_apply(self._h, b, C.byref(cost) if want_cost else None, self._stream()), "avae_dp_apply")
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
        mu = self._new(rows, self.n_z)
        lv = torch.empty_like(mu) if want_logvar else None
        if rows:
            _capi.check(self._h, self._L.avae_encode(self._h, m, t.data_ptr(), ld_of(t), rows, mu.data_ptr(), ptr(lv),
                                                     self._stream()), "avae_encode")
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

    # ------------------------------------------------------------------ cross-modal retrieval
    def posterior(self, X, sens_idx=None):
        """``transform`` with the spread: the posterior ``(mu, logvar)`` of each modality, ``[rows, n_z]`` each -- what
        ``latent_topk`` takes as a query or a gallery.  ``sens_idx`` is None (X = list over modalities, returns a list of pairs)
        or an integer (X = one array, returns one pair).  ``mu`` is bitwise ``transform``'s output."""
        if sens_idx is None:
            return [self._encode(m, x, want_logvar=True) for m, x in enumerate(X)]
        assert sens_idx < len(self.network_architectures)
        return self._encode(sens_idx, X, want_logvar=True)

    def latent_topk(self, query, gallery, k=1, metric="symkl"):
        """The ``k`` nearest gallery posteriors of every query posterior, in one fused pass on the device (avae_latent_topk in
        include/avae.h): the [N, G] distance matrix is never formed.

        ``query`` and ``gallery`` are ``(mu, logvar)`` pairs as ``posterior`` returns them (``logvar`` may be None for
        ``metric="l2"``).  ``metric="symkl"`` is KL(q_n || q_g) + KL(q_g || q_n), the divergence the association term trains on;
        ``"l2"`` the squared distance of the means.  ``1 <= k <= 64``.  Returns ``dict(index=[N, k] int32, distance=[N, k]
        float32)``, each row in ascending (isnan(distance), distance, index) order; ``k`` beyond the gallery pads with index -1,
        distance +inf.  NumPy in gives NumPy out, tensors in give device tensors out."""
        qm, ql, gm, gl, k, mid, was_np = topk_args(query, gallery, k, metric, self.n_z, self.device)
        rows = qm.shape[0]
        index = torch.empty((rows, k), dtype=torch.int32, device=self.device)
        dist = self._new(rows, k)
        if rows:
            _capi.check(self._h, self._L.avae_latent_topk(self._h, qm.data_ptr(), ptr(ql), rows, gm.data_ptr(), ptr(gl), gm.shape[0],
                                                          mid, k, index.data_ptr(), dist.data_ptr(), self._stream()),
                        "avae_latent_topk")
        conv = self._like_input(was_np)
        return {"index": conv(index), "distance": conv(dist)}

    def retrieve(self, X, sens_idx, gallery, k=1, metric="symkl"):
        """Encode the rows ``X`` of modality ``sens_idx`` and look their posteriors up in ``gallery`` (a ``(mu, logvar)`` pair,
        usually ``posterior`` of another modality's stored examples): ``latent_topk(posterior(X, sens_idx), gallery, k, metric)``."""
        return self.latent_topk(self.posterior(X, sens_idx), gallery, k=k, metric=metric)

    def retrieval_recall(self, X, ks=(1, 5, 10), metric="symkl"):
        """Cross-modal recall@k of paired rows: ``X`` is a list over modalities with equal row counts, row n of every modality
        belonging together.  Returns ``[M, M, len(ks)]`` float64: entry (s, d, i) is the share of rows n whose own partner --
        row n of modality d's posteriors -- is among the ``ks[i]`` nearest of the query from modality s.  The diagonal is the
        trivial self-retrieval (1.0 wherever the rows' posteriors are distinct).  ``max(ks) <= 64``."""
        ks = [int(k) for k in ks]
        if not ks or min(ks) < 1 or max(ks) > _capi.TOPK_MAX:
            raise ValueError("ks must hold integers in [1, %d], got %r" % (_capi.TOPK_MAX, ks))
        ts, rows, _, _, _ = dev_modalities(X, self._widths, self.device)
        post = [self._encode(m, t, want_logvar=True) for m, t in enumerate(ts)]
        M = len(post)
        out = np.zeros((M, M, len(ks)), dtype=np.float64)
        if not rows:
            return out
        own = torch.arange(rows, dtype=torch.int32, device=self.device)[:, None]
        for s_ in range(M):
            for d in range(M):
                idx = self.latent_topk(post[s_], post[d], k=max(ks), metric=metric)["index"]
                hit = idx == own                                     # [N, kmax]: at most one True per row
                for i, k in enumerate(ks):
                    out[s_, d, i] = float(hit[:, :k].any(dim=1).double().mean().item())
        return out

    # ------------------------------------------------------------------ posterior diagnostics
    STATS_SHAPES = (("count", "MM"), ("mean", "MMz"), ("var", "MMz"), ("xcov", "MMz"), ("assoc", "MMz"), ("post_var", "Mz"),
                    ("kl", "Mz"), ("cov", "Mzz"))

    def latent_stats(self, posteriors, present=None):
        """Per-dimension statistics of a data set's posteriors, in one fused pass on the device (avae_latent_stats in
        include/avae.h): which latent dimensions are alive, where the encoders agree, how far the aggregate posterior is from the
        prior.

        ``posteriors`` is a list over modalities of ``(mu, logvar)`` pairs as ``posterior`` returns them, or None for a modality
        absent everywhere; ``present`` an [N, M] bool / integer array or tensor, or None (every given modality on every row).
        With R_sd the rows that have both s and d, returns a dict of float64 arrays (and one int64 count), population form:
        ``count [M, M]`` = |R_sd|; ``mean`` / ``var [M, M, n_z]`` of mu_s over R_sd (``var[m, m]`` is the active-units statistic);
        ``xcov [M, M, n_z]`` the covariance of mu_s and mu_d; ``assoc [M, M, n_z]`` the mean per-dimension symmetric KL of the two
        posteriors; ``post_var`` / ``kl [M, n_z]`` the mean of exp(logvar_m) and of the per-dimension KL to the prior;
        ``cov [M, n_z, n_z]`` the covariance matrix of mu_m.  An empty set gives count 0 and NaN.  The result is bit-reproducible
        and its accuracy does not depend on |mean| / std.  NumPy in gives NumPy out, tensors in give device tensors out."""
        mus, lvs, rows, p, was_np = latent_stats_args(posteriors, present, self.n_z, self.device)
        dims = {"M": len(mus), "z": self.n_z}
        res = {name: torch.empty([dims[c] for c in shape], dtype=torch.int64 if name == "count" else torch.float64, device=self.device)
               for name, shape in self.STATS_SHAPES}
        out = _capi.LatentStatsOut(**{name: t.data_ptr() for name, t in res.items()})
        _capi.check(self._h, self._L.avae_latent_stats(self._h, len(mus), self._ptrs(mus), self._ptrs(lvs), ptr(p), rows,
                                                       C.byref(out), self._stream()), "avae_latent_stats")
        conv = self._like_input(was_np)
        return {name: conv(t) for name, t in res.items()}

    def latent_diagnostics(self, X, present=None, au_threshold=0.01):
        """Encode ``X`` (a list over modalities; ``X[m] = None`` is a modality absent everywhere) and diagnose the posteriors:
        ``latent_stats`` of them plus ``active [M, n_z]`` bool = ``var[m, m] > au_threshold`` (the active units of Burda et al.),
        ``active_units [M]`` their number, ``corr [M, M, n_z]`` = ``xcov[s, d] / sqrt(var[s, d] * var[d, s])`` (NaN where a
        variance is 0) and ``agg_cov [M, n_z, n_z]`` = ``cov + diag(post_var)``, the aggregate posterior's covariance.  Inside
        ``with model.averaged():`` it diagnoses the averaged encoders."""
        if len(X) != len(self._widths):
            raise ValueError("expected a list of %d modalities, got %d" % (len(self._widths), len(X)))
        post, was_np = [], None
        for m, x in enumerate(X):
            if x is None:
                post.append(None)
                continue
            t, np_in = dev_array(x, self._widths[m], self.device)
            was_np = np_in if was_np is None else was_np
            post.append(self._encode(m, t, want_logvar=True))
        st = self.latent_stats(post, None if present is None else dev_flags(present, len(X), self.device))
        M = len(X)
        own = st["var"][torch.arange(M), torch.arange(M)]
        st["active"] = own > au_threshold
        st["active_units"] = st["active"].sum(dim=1)
        prod = st["var"] * st["var"].transpose(0, 1)
        st["corr"] = torch.where(prod > 0, st["xcov"] / torch.sqrt(prod), torch.full_like(prod, float("nan")))
        st["agg_cov"] = st["cov"] + torch.diag_embed(st["post_var"])
        conv = self._like_input(not torch.is_tensor(present) if was_np is None else was_np)
        return {name: conv(t) for name, t in st.items()}

    # ------------------------------------------------------------------ aggregate posterior
    def aggregate_log_density(self, z, gallery, exclude=None, marginals=True):
        """``log q_agg(z)`` of every row of ``z`` under the aggregate posterior of a gallery, ``q_agg(z) = 1/G sum_g q(z | x_g)``,
        in one fused pass on the device (avae_agg_logpdf in include/avae.h): the [N, G, n_z] tensor of exponents is never formed.

        ``z`` is ``[N, n_z]``; ``gallery`` a ``(mu, logvar)`` pair as ``posterior`` returns it; ``exclude`` None or ``[N]``
        integers: gallery row ``exclude[n]`` is left out of query n's mixture (leave-one-out; a value outside ``[0, G)`` leaves
        nothing out).  Returns ``dict(joint=[N] float32, marginal=[N, n_z] float32)``: the log-density of the mixture and of its
        per-dimension marginals; ``marginal`` is None with ``marginals=False``, which skips most of the work.  An empty mixture
        gives NaN.  The result is bit-reproducible and a query's value does not depend on the other queries.  NumPy in gives
        NumPy out, tensors in give device tensors out."""
        zt, gm, gl, ex, marg, was_np = agg_args(z, gallery, exclude, marginals, self.n_z, self.device)
        rows = zt.shape[0]
        joint = torch.empty((rows,), dtype=torch.float32, device=self.device)
        marginal = self._new(rows, self.n_z) if marg else None
        if rows:
            _capi.check(self._h, self._L.avae_agg_logpdf(self._h, zt.data_ptr(), rows, ptr(gm), ptr(gl), gm.shape[0], ptr(ex),
                                                         joint.data_ptr(), ptr(marginal), self._stream()), "avae_agg_logpdf")
        conv = self._like_input(was_np)
        return {"joint": conv(joint), "marginal": conv(marginal) if marg else None}

    def elbo_decomposition(self, X, n_samples=1, eps=None, seed=0, leave_one_out=False):
        """Where the KL term of the ELBO goes (Hoffman & Johnson 2016; Chen et al. 2018): per modality,
        ``kl = mi + tc + sum_j dimwise_kl`` with the aggregate posterior ``q_agg^m`` of the rows of ``X[m]`` -- plus how far apart
        the encoders' aggregate posteriors are.

        ``X`` is a list over modalities with equal row counts N; ``X[m] = None`` makes that modality's entries NaN.  Every given
        modality is encoded once; ``z^m = mu_m + exp(0.5 logvar_m) * eps`` for ``n_samples`` draws per row, ``eps``
        ``[n_samples, N, n_z]`` shared by the modalities as a training step shares its draw (None: drawn on the device from
        ``seed``).  Returns float64, means over the ``n_samples * N`` samples:
        ``kl [M]`` of ``log q(z|x) - log p(z)``; ``mi [M]`` of ``log q(z|x) - log q_agg(z)``, the index-code mutual information;
        ``tc [M]`` of ``log q_agg(z) - sum_j log q_agg,j(z_j)``, the total correlation; ``dimwise_kl [M, n_z]`` of
        ``log q_agg,j(z_j) - log p(z_j)``; ``marginal_kl [M]`` = ``tc + sum_j dimwise_kl``, the estimate of KL(q_agg || p);
        ``cross [M, M]``: ``cross[s, d]`` the mean of ``log q_agg^s(z^s) - log q_agg^d(z^s)``, the estimate of
        KL(q_agg^s || q_agg^d), diagonal exactly 0; ``log_n`` = log N.

        Without ``leave_one_out`` the mixture counts the sample's own posterior: the standard form of the estimator, biased
        towards ``mi -> log N`` (its ceiling) when the posteriors hardly overlap.  ``leave_one_out=True`` leaves row n's own
        posterior out of the mixtures its samples are scored under.  Inside ``with model.averaged():`` it decomposes the averaged
        encoders; on a data-parallel replica it covers the local rows."""
        if isinstance(n_samples, bool) or not isinstance(n_samples, (int, np.integer)) or n_samples < 1:
            raise ValueError("n_samples must be an integer >= 1, got %r" % (n_samples,))
        S, nz = int(n_samples), self.n_z
        ts, N, was_np, _, _ = dev_modalities(X, self._widths, self.device, allow_none=True)
        if N is None:
            raise ValueError("every modality is None: the row count is unknown")
        e = dev_dense3(eps, (S, N, nz), self.device)
        if e is None:
            gen = torch.Generator(device=self.device)
            gen.manual_seed(int(seed))
            e = torch.randn((S, N, nz), generator=gen, device=self.device, dtype=torch.float32)
        M, c = len(ts), 0.5 * float(np.log(2.0 * np.pi))
        post = [None if t is None else self._encode(m, t, want_logvar=True) for m, t in enumerate(ts)]
        own = torch.arange(N, dtype=torch.int32, device=self.device).repeat(S) if leave_one_out else None
        nan = float("nan")
        a = torch.full((M,), nan, dtype=torch.float64, device=self.device)          # mean log q(z|x)
        b = torch.full((M, M), nan, dtype=torch.float64, device=self.device)        # b[s, d]: mean log q_agg^d(z^s)
        cj = torch.full((M, nz), nan, dtype=torch.float64, device=self.device)      # mean log q_agg,j^s(z^s_j)
        pj = torch.full((M, nz), nan, dtype=torch.float64, device=self.device)      # mean log p(z^s_j)
        e64 = e.double()
        for s_ in range(M):
            if post[s_] is None:
                continue
            mu, lv = post[s_][0].double(), post[s_][1].double()
            z64 = (mu[None] + torch.exp(0.5 * lv)[None] * e64).reshape(S * N, nz)
            z = z64.float()
            a[s_] = (-0.5 * e64 * e64 - 0.5 * lv[None] - c).sum(dim=2).mean() if S * N else nan
            pj[s_] = (-0.5 * z64 * z64 - c).mean(dim=0)
            for d in range(M):
                if post[d] is None:
                    continue
                r = self.aggregate_log_density(z, post[d], exclude=own, marginals=(d == s_))
                b[s_, d] = r["joint"].double().mean()
                if d == s_:
                    cj[s_] = r["marginal"].double().mean(dim=0)
        own_b = torch.diagonal(b)
        out = {"kl": a - pj.sum(dim=1), "mi": a - own_b, "tc": own_b - cj.sum(dim=1), "dimwise_kl": cj - pj}
        out["marginal_kl"] = out["tc"] + out["dimwise_kl"].sum(dim=1)
        out["cross"] = own_b[:, None] - b
        conv = self._like_input(bool(was_np))
        out = {name: conv(t) for name, t in out.items()}
        out["log_n"] = float(np.log(N)) if N else float("-inf")
        return out

    # ------------------------------------------------------------------ mixture prior
    def _gmm_fit(self, mu, lv, K, n_iters, var_floor, w, m, s):
        """avae_gmm_fit in place on the contiguous float32 device tensors ``w``, ``m``, ``s`` -> (bound [n_iters + 1] float64,
        n_used [1] int32), device tensors"""
        bound = torch.empty((n_iters + 1,), dtype=torch.float64, device=self.device)
        n_used = torch.empty((1,), dtype=torch.int32, device=self.device)
        _capi.check(self._h, self._L.avae_gmm_fit(self._h, ptr(mu), ptr(lv), mu.shape[0], K, n_iters, var_floor, w.data_ptr(),
                                                  m.data_ptr(), s.data_ptr(), bound.data_ptr(), n_used.data_ptr(), self._stream()),
                    "avae_gmm_fit")
        return bound, n_used

    def fit_latent_prior(self, posteriors, n_components=10, n_iters=50, init=None, seed=0, var_floor=1e-6):
        """Fit a diagonal Gaussian mixture ``p(z) = sum_k pi_k N(z; m_k, diag exp(s_k))`` to posteriors, on the device
        (avae_gmm_fit in include/avae.h): the prior to sample from instead of N(0, I) once the aggregate posterior is a handful of
        clusters with holes between them (ex-post density estimation), and an unsupervised clustering of the codes.

        ``posteriors`` is a ``(mu, logvar)`` pair as ``posterior`` returns it, or a list of such pairs whose rows are concatenated
        -- one prior for every encoder's codes, the one ``generate`` decodes for all modalities.  ``logvar`` may be None (points:
        textbook EM); with it the fit maximises the Jensen bound of ``mean_n E_{q_n}[log p(z)]``.  ``1 <= n_components <= 64``;
        ``n_iters`` EM iterations, no early stop.  ``init=None`` starts the means at ``n_components`` rows picked by
        ``np.random.default_rng(seed).permutation`` over the rows without a non-finite entry, every log-variance at the data's total
        per-dimension variance and the weights at 1/K; or ``init=dict(weights=, means=, logvars=)`` to warm-start.  A row with a
        non-finite entry is skipped; a component that loses all its rows keeps its place with weight 0.

        Returns ``dict(weights [K], means [K, n_z], logvars [K, n_z] float32, bound [n_iters + 1] float64, n_used int)``:
        ``bound[t]`` is the bound of the parameters entering iteration t, ``bound[-1]`` that of the returned ones.  The result is
        bit-reproducible, and a fit continued from its own output gives the bits of the longer fit.  NumPy in gives NumPy out,
        tensors in give device tensors out."""
        mu, lv, K, T, vf, start, seed_rows, was_np = latent_prior_args(posteriors, n_components, n_iters, init, seed, var_floor,
                                                                       self.n_z, self.device)
        if start is None:
            m = mu[seed_rows.to(self.device)].contiguous()
            w1 = torch.ones((1,), dtype=torch.float32, device=self.device)
            m1, s1 = m[:1].clone(), torch.zeros((1, self.n_z), dtype=torch.float32, device=self.device)
            self._gmm_fit(mu, lv, 1, 1, vf, w1, m1, s1)             # one K = 1 iteration: s1 = log of the total variance
            w = torch.full((K,), 1.0 / K, dtype=torch.float32, device=self.device)
            s = s1.expand(K, self.n_z).contiguous()
        else:
            w, m, s = start
        bound, n_used = self._gmm_fit(mu, lv, K, T, vf, w, m, s)
        conv = self._like_input(was_np)
        return {"weights": conv(w), "means": conv(m), "logvars": conv(s), "bound": conv(bound), "n_used": int(n_used.item())}

    def latent_prior_score(self, z, prior, responsibilities=False):
        """Score rows under a mixture prior (avae_gmm_score in include/avae.h).  ``z`` is a ``[N, n_z]`` array (points) or a
        ``(mu, logvar)`` pair; ``prior`` a dict of ``weights``, ``means``, ``logvars`` as ``fit_latent_prior`` returns it.
        Returns ``dict(log_density [N] float32, component [N] int32, responsibilities [N, K] float32 or None)``: for points
        ``log_density`` is exactly ``log p(z)`` -- a novelty score against K components instead of a whole gallery -- for pairs the
        per-row term of the fit's bound; ``component`` is the most responsible component (ties to the lower index).  A row with
        a non-finite entry gives NaN, -1 and NaN.  A row's result does not depend on the other rows."""
        mu, lv, w, m, s, was_np = latent_score_args(z, prior, self.n_z, self.device)
        rows, K = mu.shape[0], w.shape[0]
        ll = torch.empty((rows,), dtype=torch.float32, device=self.device)
        comp = torch.empty((rows,), dtype=torch.int32, device=self.device)
        resp = self._new(rows, K) if responsibilities else None
        if rows:
            _capi.check(self._h, self._L.avae_gmm_score(self._h, mu.data_ptr(), ptr(lv), rows, K, w.data_ptr(), m.data_ptr(),
                                                        s.data_ptr(), ll.data_ptr(), comp.data_ptr(), ptr(resp), self._stream()),
                        "avae_gmm_score")
        conv = self._like_input(was_np)
        return {"log_density": conv(ll), "component": conv(comp), "responsibilities": conv(resp) if responsibilities else None}

    def sample_latent_prior(self, prior, n, seed=0):
        """``n`` draws ``[n, n_z]`` from a mixture prior: the component from ``weights``, then its Gaussian, with a device generator
        seeded by ``seed``.  ``generate(sample_latent_prior(prior, 64))`` replaces ``generate(None)``'s N(0, I) draw.  NumPy
        prior gives NumPy out, a tensor prior device tensors."""
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0:
            raise ValueError("n must be an integer >= 0, got %r" % (n,))
        w, m, s, was_np = prior_arrays(prior, self.n_z, self.device)
        gen = torch.Generator(device=self.device)
        gen.manual_seed(int(seed))
        if n:
            comp = torch.multinomial(w.double(), int(n), replacement=True, generator=gen)
        else:
            comp = torch.empty((0,), dtype=torch.int64, device=self.device)
        eps = torch.randn((int(n), self.n_z), generator=gen, device=self.device, dtype=torch.float32)
        z = m[comp] + torch.exp(0.5 * s[comp]) * eps
        return self._like_input(was_np)(z)

    # ------------------------------------------------------------------ 2-D map of the posteriors
    def embed_latents(self, posteriors, perplexity=30.0, n_iters=1000, metric="symkl", learning_rate="auto", early_exaggeration=12.0,
                      exaggeration_iters=250, momentum=(0.5, 0.8), init=None, seed=0, state=None):
        """A 2-D t-SNE map of posteriors, computed on the device (avae_embed_calibrate / avae_embed_iterate in include/avae.h):
        where the codes lie, as a picture.  The N x N affinities are never stored; the sums are exact (no Barnes-Hut) and the
        result is bit-reproducible.

        ``posteriors`` is a ``(mu, logvar)`` pair as ``posterior`` returns it, or a list of such pairs whose rows are concatenated
        into one map.  ``metric="symkl"`` builds the affinities from KL(q_i || q_j) + KL(q_j || q_i), the divergence the
        association term trains on (variances included); ``"l2"`` from the squared distance of the means (``logvar`` may then be
        None).  ``learning_rate="auto"`` is ``max(F / 48, 50)``; ``init=None`` starts at
        ``np.random.default_rng(seed).normal(0, 1e-4, (N, 2))``.  A row with a non-finite entry is skipped and comes back NaN.
        At most 65,536 rows.

        Returns ``dict(embedding [N, 2] float32, kl [n_iters + 1] float64, beta [N] float32, n_used int, state)``: ``kl[s]`` is
        the divergence of the map entering iteration s, ``kl[-1]`` that of the returned one (centred on the used rows' mean);
        ``state`` (embedding, velocity, gains, iteration, calibration) passed back as ``state=`` continues the run for
        ``n_iters`` more iterations without calibrating again.  NumPy in gives NumPy out, tensors in give device tensors out."""
        a = embed_args(posteriors, perplexity, n_iters, metric, learning_rate, early_exaggeration, exaggeration_iters, momentum, init,
                       seed, state, self.n_z, self.device)
        mu, lv, N = a["mu"], a["logvar"], a["rows"]
        if a["calibration"] is None:
            beta, shift, norm = (torch.empty((N,), dtype=torch.float32, device=self.device) for _ in range(3))
            tries = torch.empty((N,), dtype=torch.int32, device=self.device)
            n_used = torch.empty((1,), dtype=torch.int32, device=self.device)
            _capi.check(self._h, self._L.avae_embed_calibrate(self._h, mu.data_ptr(), ptr(lv), N, a["metric"], a["perplexity"], 1e-5, 64,
                                                              beta.data_ptr(), shift.data_ptr(), norm.data_ptr(), tries.data_ptr(),
                                                              n_used.data_ptr(), self._stream()), "avae_embed_calibrate")
        else:
            beta, shift, norm = a["calibration"]
        y, vel, gain, T = a["y"], a["vel"], a["gain"], a["n_iters"]
        kl = torch.empty((T + 1,), dtype=torch.float64, device=self.device)
        _capi.check(self._h, self._L.avae_embed_iterate(self._h, mu.data_ptr(), ptr(lv), N, a["metric"], beta.data_ptr(), shift.data_ptr(),
                                                        norm.data_ptr(), y.data_ptr(), vel.data_ptr(), gain.data_ptr(), a["it0"], T,
                                                        a["learning_rate"], a["early_exaggeration"], a["exaggeration_iters"],
                                                        a["momentum"][0], a["momentum"][1], 1, kl.data_ptr(), None, self._stream()),
                    "avae_embed_iterate")
        conv = self._like_input(a["was_numpy"])
        out_state = {"embedding": conv(y), "velocity": conv(vel), "gains": conv(gain), "iteration": a["it0"] + T,
                     "beta": conv(beta), "shift": conv(shift), "norm": conv(norm)}
        return {"embedding": out_state["embedding"], "kl": conv(kl), "beta": out_state["beta"], "n_used": a["n_used"], "state": out_state}

    def latent_map(self, X, **kw):
        """Encode every modality of ``X`` (a list over modalities with equal row counts N) with ``posterior`` and embed all M * N
        codes in ONE map (``embed_latents``, which takes ``kw``): the reference's picture of associated encodings -- paired rows
        of a well-associated model land on each other.  Returns ``embed_latents``' dict with ``embedding`` reshaped to
        ``[M, N, 2]``: ``embedding[m, n]`` is where modality m's code of row n lies.  Inside ``with model.averaged():`` it maps the
        averaged encoders' codes."""
        ts, rows, was_np, _, _ = dev_modalities(X, self._widths, self.device)
        post = [self._encode(m, t, want_logvar=True) for m, t in enumerate(ts)]
        out = self.embed_latents(post, **kw)
        conv = self._like_input(bool(was_np))
        out = {k: (conv(v) if torch.is_tensor(v) else v) for k, v in out.items()}
        out["state"] = {k: (conv(v) if torch.is_tensor(v) else v) for k, v in out["state"].items()}
        out["embedding"] = out["embedding"].reshape(len(post), rows, 2)
        return out

    def generate(self, z_mu=None):
        """Generate data by sampling from latent space: decoder only, z fed directly; returns the
        list of per-modality decoder means.  ``None`` draws z from the prior with NumPy's global
        RNG, batch_size rows (reference vae_assoc.py:405-419)."""
        if z_mu is None:
            z_mu = np.random.normal(size=(self.batch_size, self.n_z))
        z = dev_dense(z_mu, self.n_z, self.device)
        rows = z.shape[0]
        outs = [self._new(rows, cols) for cols in self._widths]
        if rows:       # every modality's decoder in one submission (avae_generate: one graph replay for 1-64 rows)
            _capi.check(self._h, self._L.avae_generate(self._h, z.data_ptr(), rows, self._ptrs(outs), self._stream()), "avae_generate")
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
            o = self._new(rows, cols)
            if rows:
                _capi.check(self._h, self._L.avae_reconstruct(self._h, m, t.data_ptr(), ld_of(t), ptr(e), rows, o.data_ptr(),
                                                              self._stream()), "avae_reconstruct")
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
        out = self._new(rows, k.value)
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
        out = self._new(rows, 2 * M + M * M)
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
        out_z, grad, obj = self._new(rows, self.n_z), self._new(rows, self.n_z), self._new(n_iters + 1, rows)
        outs = [self._new(rows, cols) for cols in widths]
        if rows:
            _capi.check(self._h, self._L.avae_complete(self._h, xp, lds, self._ptrs(obs), z.data_ptr(), rows, n_iters, float(lr),
                                                       float(prior_weight), out_z.data_ptr(), obj.data_ptr(), grad.data_ptr(),
                                                       self._ptrs(outs), self._stream()), "avae_complete")
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
        mu, lv = self._new(rows, self.n_z), self._new(rows, self.n_z)
        mean = [self._new(rows, cols) for cols in widths]
        var = [self._new(rows, cols) for cols in widths] if K else None
        if rows:
            _capi.check(self._h, self._L.avae_impute(self._h, xp, lds, ptr(p), rows, K, ptr(e), mu.data_ptr(), lv.data_ptr(),
                                                     self._ptrs(mean), self._ptrs(var) if K else None, self._stream()), "avae_impute")
        conv = self._like_input(was_np)
        return {"mu": conv(mu), "logvar": conv(lv), "mean": [conv(o) for o in mean],
                "var": [conv(o) for o in var] if K else None}

    # ------------------------------------------------------------------ motion decoding
    _motion_chunk = 16384      # decoded rows (input rows x samples) predict_motion holds at a time

    def _motion_eval(self, p, mats, basis, ref=None, refp=None):
        """avae_motion_eval on device tensors -> (trajectory [N, T, D], saturated [N, D] int32, rmse, max_abs [N, D] or None)"""
        N, T, D = p.shape[0], basis.n_points, basis.n_dof
        traj = torch.empty((N, T, D), dtype=torch.float32, device=self.device)
        sat = torch.empty((N, D), dtype=torch.int32, device=self.device)
        has_ref = ref is not None or refp is not None
        rmse, mx = (self._new(N, D), self._new(N, D)) if has_ref else (None, None)
        if N:
            _capi.check(self._h, self._L.avae_motion_eval(
                self._h, p.data_ptr(), N, D, basis.n_kb, T, mats["phi"].data_ptr(), ptr(mats["scale"]), ptr(mats["shift"]),
                ptr(mats["limits"]), ptr(mats["gain"]), ptr(mats["target"]), mats["nc"], ptr(ref), ptr(refp),
                traj.data_ptr(), sat.data_ptr(), ptr(rmse), ptr(mx), self._stream()), "avae_motion_eval")
        return traj, sat, rmse, mx

    def motion_eval(self, params, basis, anchor=None, reference=None, reference_params=None):
        """Standardised approximator parameters -> joint trajectories (avae_motion_eval in include/avae.h): what the reference does
        after every ``generate`` (baxter_vae_assoc_writer.py:145-150, 439-458) -- un-normalise with the basis' ``param_mean`` /
        ``param_std``, evaluate every joint's approximator at the basis' phase points, clamp to the joint limits.

        ``params`` is ``[N, basis.n_params]``; ``anchor`` None or ``dict(phases=[...], target=[N, n_dof, n_c])``: the trajectory
        of the parameters projected onto passing through ``target`` at ``phases`` (pyrbf_funcapprox.py:41-61).  ``reference``
        (``[N, n_points, n_dof]`` trajectories) or ``reference_params`` (``[N, n_params]``, evaluated the same way, without
        anchor) asks for the error against it.  Returns a dict: ``trajectory [N, n_points, n_dof]``, ``saturated [N, n_dof]``
        (int32, the number of clamped points) and ``rmse`` / ``max_abs [N, n_dof]`` over the time points (None without a
        reference).  NumPy in gives NumPy out, device tensors in give device tensors out."""
        p, mats, ref, refp, was_np = motion_eval_args(params, basis, anchor, reference, reference_params, self.device)
        traj, sat, rmse, mx = self._motion_eval(p, mats, basis, ref, refp)
        conv = self._like_input(was_np)
        return {"trajectory": conv(traj), "saturated": conv(sat), "rmse": None if rmse is None else conv(rmse),
                "max_abs": None if mx is None else conv(mx)}

    def motion_fit(self, trajectories, basis):
        """Joint trajectories ``[N, T, n_dof]`` -> standardised parameters ``[N, basis.n_params]`` (avae_motion_fit): the
        least-squares fit of the basis at ``linspace(0, 1, T)`` with the reference's truncated pseudo-inverse, per joint, then
        ``(theta - param_mean) / param_std`` (baxter_writer.py:77-82, 193).  T is the input's own."""
        t, pinv, sc, sh, was_np = motion_fit_args(trajectories, basis, self.device)
        return self._like_input(was_np)(self._motion_fit(t, pinv, sc, sh, basis))

    def _motion_fit(self, t, pinv, sc, sh, basis):
        """avae_motion_fit on device tensors: trajectories [N, T, D] -> standardised parameters [N, P]"""
        N, T = t.shape[0], t.shape[1]
        out = self._new(N, basis.n_params)
        if N:
            _capi.check(self._h, self._L.avae_motion_fit(self._h, t.data_ptr(), N, basis.n_dof, basis.n_kb, T, pinv.data_ptr(),
                                                         ptr(sc), ptr(sh), out.data_ptr(), self._stream()), "avae_motion_fit")
        return out

    def _motion_moments(self, s, N, S, mats, basis, mean, var, frac):
        """avae_motion_moments on N rows of S dense samples at ``s`` into (slices of) the outputs"""
        _capi.check(self._h, self._L.avae_motion_moments(
            self._h, s.data_ptr(), N, S, basis.n_dof, basis.n_kb, basis.n_points, mats["phi"].data_ptr(), ptr(mats["scale"]),
            ptr(mats["shift"]), ptr(mats["limits"]), ptr(mats["gain"]), ptr(mats["target"]), mats["nc"],
            mean.data_ptr(), ptr(var), ptr(frac), self._stream()), "avae_motion_moments")

    def motion_moments(self, samples, basis, anchor=None):
        """Per-point mean and population variance of the trajectories of S parameter samples per row (avae_motion_moments):
        ``samples`` is ``[N, S, basis.n_params]``, every sample evaluated as by ``motion_eval`` (clamp included) and folded into
        running moments on the device; the ``N S n_points n_dof`` trajectory values are never stored.  Returns a dict: ``mean`` and
        ``var [N, n_points, n_dof]`` and ``saturated_frac [N, n_dof]``, the share of clamped points over samples and time."""
        s, mats, was_np = motion_moments_args(samples, basis, anchor, self.device)
        N, S = s.shape[0], s.shape[1]
        shape = (N, basis.n_points, basis.n_dof)
        mean, var = (torch.empty(shape, dtype=torch.float32, device=self.device) for _ in range(2))
        frac = self._new(N, basis.n_dof)
        if N:
            self._motion_moments(s, N, S, mats, basis, mean, var, frac)
        conv = self._like_input(was_np)
        return {"mean": conv(mean), "var": conv(var), "saturated_frac": conv(frac)}

    def _fused_decode(self, xp, lds, p, rows, modality, want_mean):
        """avae_impute with no samples -> (mu, logvar, the decoded fused mean of ``modality`` or None)"""
        mu, lv = self._new(rows, self.n_z), self._new(rows, self.n_z)
        mean = [None] * len(self._widths)
        if want_mean:
            mean[modality] = self._new(rows, self._widths[modality])
        if rows:
            _capi.check(self._h, self._L.avae_impute(self._h, xp, lds, ptr(p), rows, 0, None, mu.data_ptr(), lv.data_ptr(),
                                                     self._ptrs(mean), None, self._stream()), "avae_impute")
        return mu, lv, mean[modality]

    def _decode(self, modality, z, out=None):
        """avae_decode on device tensors: latents ``z [rows, n_z]`` -> the parameters of ``modality`` (into ``out`` if given)"""
        if out is None:
            out = self._new(z.shape[0], self._widths[modality])
        if z.shape[0]:
            _capi.check(self._h, self._L.avae_decode(self._h, modality, z.data_ptr(), z.shape[0], out.data_ptr(), self._stream()),
                        "avae_decode")
        return out

    def predict_motion(self, X, basis, modality=1, present=None, n_samples=0, eps=None, anchor=None):
        """From the modalities each row has to the joint trajectory of modality ``modality`` (the writer's
        ``derive_robot_motion_from_img``, baxter_vae_assoc_writer.py:439-458, up to the trajectory): ``impute``'s fused posterior,
        decoded and evaluated with ``basis`` (``basis.n_params`` must be the modality's ``n_input``).

        ``X`` / ``present`` as in ``impute``.  ``n_samples = 0``: the trajectory of the decoded fused mean, bitwise
        ``motion_eval(impute(X, present)["mean"][modality], basis, anchor)``.  ``n_samples = S >= 1``: the per-point mean and
        population variance over the trajectories of S samples ``z = mu + exp(logvar / 2) eps`` (``eps`` [N, S, n_z], or None for
        a fresh draw from torch's generator), computed in row chunks: a chunk's latents are decoded and their trajectories
        folded into the moments on the device, so only one chunk's decoded parameters ever exist.

        Returns a dict: ``mu``, ``logvar [N, n_z]``, ``trajectory [N, n_points, n_dof]`` (with samples: their mean), ``var``
        (None without samples) and ``saturated_frac [N, n_dof]``, the share of clamped points."""
        (ts, rows, was_np, xp, lds, p, S, e), mats = predict_motion_args(X, basis, modality, present, n_samples, eps, anchor,
                                                                         self._widths, self.n_z, self.device)
        conv = self._like_input(was_np)
        mu, lv, mean = self._fused_decode(xp, lds, p, rows, modality, S == 0)
        out = {"mu": conv(mu), "logvar": conv(lv), "var": None}
        if S == 0:
            traj, sat, _, _ = self._motion_eval(mean, mats, basis)
            out.update(trajectory=conv(traj), saturated_frac=conv(sat.to(torch.float32) / float(basis.n_points)))
            return out
        shape = (rows, basis.n_points, basis.n_dof)
        traj, var = (torch.empty(shape, dtype=torch.float32, device=self.device) for _ in range(2))
        frac = self._new(rows, basis.n_dof)
        if e is None:
            e = torch.randn((rows, S, self.n_z), dtype=torch.float32, device=self.device)
        sd = torch.exp(0.5 * lv)
        chunk = max(1, int(self._motion_chunk) // S)
        dec = self._new(min(chunk, rows) * S, basis.n_params)
        target = mats["target"]
        for r0 in range(0, rows, chunk):
            n = min(chunk, rows - r0)
            z = (mu[r0:r0 + n, None, :] + sd[r0:r0 + n, None, :] * e[r0:r0 + n]).reshape(n * S, self.n_z).contiguous()
            self._decode(modality, z, dec)
            m = dict(mats, target=None if target is None else target[r0:r0 + n])
            self._motion_moments(dec, n, S, m, basis, traj[r0:r0 + n], var[r0:r0 + n], frac[r0:r0 + n])
        out.update(trajectory=conv(traj), var=conv(var), saturated_frac=conv(frac))
        return out

    def motion_error(self, X, basis, source=0, modality=1):
        """The cross-modal prediction error in joint units: the trajectory decoded from the posterior mean of modality ``source``
        against the trajectory of the row's own parameters ``X[modality]``, both evaluated with ``basis``.  Returns a dict of
        ``rmse`` and ``max_abs [N, n_dof]`` over the time points -- ``motion_eval(impute(only source)["mean"][modality], basis,
        reference_params=X[modality])``."""
        M = len(self._widths)
        as_index(source, "source", M)
        if len(X) != M:
            raise ValueError("expected a list of %d modalities, got %d" % (M, len(X)))
        only = [X[m] if m == source else None for m in range(M)]
        (ts, rows, was_np, xp, lds, p, _, _), mats = predict_motion_args(only, basis, modality, None, 0, None, None, self._widths,
                                                                        self.n_z, self.device)
        if X[modality] is None:
            raise ValueError("X[%d] is None: the error needs the row's own parameters" % modality)
        refp = dev_dense(X[modality], basis.n_params, self.device, rows, "as X[%d]" % source, name="X[%d]" % modality)
        _, _, mean = self._fused_decode(xp, lds, p, rows, modality, True)
        _, _, rmse, mx = self._motion_eval(mean, mats, basis, None, refp)
        conv = self._like_input(was_np)
        return {"rmse": conv(rmse), "max_abs": conv(mx)}

    # ------------------------------------------------------------------ pen path and drawing
    def _motion_fk(self, t, frames, axes):
        """avae_motion_fk on device tensors: trajectories [N, T, D] -> pen path [N, T, 3]"""
        N, T, D = t.shape
        path = torch.empty((N, T, 3), dtype=torch.float32, device=self.device)
        if N:
            _capi.check(self._h, self._L.avae_motion_fk(self._h, t.data_ptr(), N, T, D, frames.data_ptr(), axes.data_ptr(),
                                                        path.data_ptr(), self._stream()), "avae_motion_fk")
        return path

    def _render(self, p, plane, canvas, target, height):
        """avae_stroke_render on device tensors -> dict of device tensors (``img_l2`` / ``height_l2`` None without their input)"""
        N, T, H = p.shape[0], p.shape[1], canvas.size
        image, window = self._new(N, H * H), self._new(N, 3)
        l2 = None if target is None else torch.empty(N, dtype=torch.float32, device=self.device)
        hl2 = None if height is None else torch.empty(N, dtype=torch.float32, device=self.device)
        if N:
            _capi.check(self._h, self._L.avae_stroke_render(
                self._h, p.data_ptr(), N, T, plane.data_ptr(), canvas.half_width, canvas.margin, H, canvas.supersample,
                ptr(target), ptr(height), image.data_ptr(), window.data_ptr(), ptr(l2), ptr(hl2), self._stream()),
                "avae_stroke_render")
        return {"image": image, "window": window, "img_l2": l2, "height_l2": hl2}

    def motion_fk(self, trajectories, chain):
        """Joint trajectories ``[N, T, chain.n_dof]`` -> the pen tip's path ``[N, T, 3]`` (avae_motion_fk in include/avae.h): the
        reference's ``derive_cartesian_trajectory`` (baxter_vae_assoc_writer.py:448-449), one launch for every row and time point
        instead of one PyKDL call per point."""
        t, frames, axes, was_np = motion_fk_args(trajectories, chain, self.device)
        return self._like_input(was_np)(self._motion_fk(t, frames, axes))

    def render_strokes(self, path, canvas, target=None, height=None):
        """Pen paths ``[N, T, 3]`` -> the pictures they write (avae_stroke_render): the path projected on the canvas' plane, drawn as
        a line of the canvas' width, cropped to its ink plus the margin and sampled to ``size x size`` pixels -- the project's own
        definition of what the reference does with matplotlib and OpenCV (``derive_img_from_robot_cart_motion``, utils.py:240-257),
        not a bit copy of it.  ``target`` (``[N, size * size]``, or one picture for every row) asks for the pixel distance,
        ``height`` (``[N]`` or one number) for the distance of the path from that height above the plane.  Returns a dict:
        ``image [N, size * size]`` (row 0 the top), ``window [N, 3]`` (centre u, v and side of the drawn window in plane units),
        ``img_l2`` and ``height_l2 [N]`` (None without their input).  A row with a non-finite path is NaN throughout."""
        p, plane, tg, hg, was_np = render_args(path, canvas, target, height, self.device)
        conv = self._like_input(was_np)
        return {k: None if v is None else conv(v) for k, v in self._render(p, plane, canvas, tg, hg).items()}

    def draw_motion(self, params, basis, chain, canvas, anchor=None, target=None, height=None):
        """Standardised approximator parameters -> the picture the motion writes: ``motion_eval``, ``motion_fk`` and
        ``render_strokes`` chained on the device.  Returns ``render_strokes``' dict with ``trajectory [N, n_points, n_dof]`` and
        ``path [N, n_points, 3]`` added; every piece is bitwise what the separate calls give."""
        p, mats, frames, axes, plane, tg, hg, was_np = draw_args(params, basis, chain, canvas, anchor, target, height, self.device)
        traj = self._motion_eval(p, mats, basis)[0]
        path = self._motion_fk(traj, frames, axes)
        out = self._render(path, plane, canvas, tg, hg)
        out.update(trajectory=traj, path=path)
        conv = self._like_input(was_np)
        return {k: None if v is None else conv(v) for k, v in out.items()}

    def writing_cost(self, params, basis, chain, canvas, target_image, target_latent=None, height=None, weights=(0.3, 10.0, 0.7),
                     image_modality=0):
        """The reference's ``cost_robot_joint_motion_fa_img`` (baxter_vae_assoc_writer.py:344-399) for N candidate motions at
        once: each row of ``params`` is drawn (``draw_motion``) and compared with ``target_image`` (``[N, n_pixels]`` or one
        picture) pixel by pixel and, after encoding the drawing with modality ``image_modality``, in latent space against
        ``target_latent`` (``[N, n_z]`` or one row; default: the encoding of ``target_image``).  ``height`` is the height the pen
        should keep (default: the row's own mean height, so a flat stroke costs nothing).
        ``cost = w0 (img_l2 + w1 height_l2) + w2 latent_l2``; returns a dict of ``cost``, ``img_l2``, ``height_l2``,
        ``latent_l2 [N]``, ``image``, ``path`` and ``trajectory``."""
        w = writing_cost_args(weights, image_modality, canvas, self._widths)
        if target_image is None:
            raise ValueError("target_image is None: the cost needs the picture to compare with")
        p, mats, frames, axes, plane, tg, hg, was_np = draw_args(params, basis, chain, canvas, None, target_image, height,
                                                                 self.device)
        rows = int(p.shape[0])
        zt = None
        if target_latent is not None:
            zt = target_latent if torch.is_tensor(target_latent) else torch.as_tensor(np.asarray(target_latent, dtype=np.float32))
            if zt.dim() == 1:
                zt = zt.reshape(1, -1).expand(rows, -1)
            zt = dev_dense(zt, self.n_z, self.device, rows, "as params", name="target_latent")
        out = self._writing_cost(p, mats, basis, frames, axes, plane, canvas, tg, hg, zt, w, image_modality)
        conv = self._like_input(was_np)
        return {k: conv(out[k]) for k in ("cost", "img_l2", "height_l2", "latent_l2", "image", "path", "trajectory")}

    def _writing_cost(self, p, mats, basis, frames, axes, plane, canvas, tg, hg, zt, w, image_modality):
        """``writing_cost`` on device tensors, with no host round trip: parameters ``p [N, P]`` and their targets (``hg`` None: the
        row's own mean height, ``zt`` None: the encoding of ``tg``) -> dict of device tensors, ``height`` (the one used) among them"""
        traj = self._motion_eval(p, mats, basis)[0]
        path = self._motion_fk(traj, frames, axes)
        if hg is None:
            hg = (path @ plane[2]).mean(1).contiguous()
        out = self._render(path, plane, canvas, tg, hg)
        if zt is None:
            zt = self._encode(image_modality, tg)
        lat = torch.linalg.vector_norm(self._encode(image_modality, out["image"]) - zt, dim=1)
        lat = torch.where(torch.isnan(out["img_l2"]), out["img_l2"], lat)      # (a row that could not be drawn)
        cost = w[0] * (out["img_l2"] + w[1] * out["height_l2"]) + w[2] * lat
        return {"cost": cost, "img_l2": out["img_l2"], "height_l2": out["height_l2"], "latent_l2": lat, "image": out["image"],
                "path": path, "trajectory": traj, "height": hg}

    # ------------------------------------------------------------------ letter thumbnails
    def _letter_thumbnails(self, t, row, frame, flags, thr, size):
        """avae_letter_thumbnail on a device uint8 tensor [N, Hf, Wf, C] -> dict of device tensors"""
        N, Hf, Wf, Cn = (int(s) for s in t.shape)
        image = self._new(N, size * size)
        box, window, ink = (torch.empty(s, dtype=torch.int32, device=self.device) for s in ((N, 4), (N, 3), (N,)))
        if N:
            need = C.c_size_t(0)
            if self._L.avae_letter_thumbnail_plan(N, Hf, Wf, None, C.byref(need)) != 0:
                raise RuntimeError("avae_letter_thumbnail_plan failed: %s" % self._L.avae_last_error(None).decode("utf-8", "replace"))
            ws = torch.empty(need.value, dtype=torch.uint8, device=self.device)
            _capi.check(self._h, self._L.avae_letter_thumbnail(
                self._h, t.data_ptr(), N, Hf, Wf, Cn, row, frame, flags, thr, size, ws.data_ptr(), need.value,
                image.data_ptr(), box.data_ptr(), window.data_ptr(), ink.data_ptr(), self._stream()), "avae_letter_thumbnail")
        return {"image": image, "box": box, "window": window, "ink": ink}

    def letter_thumbnails(self, frames, size=28, threshold=None, invert=False, channel_order="rgb"):
        """Camera frames or drawing-pad canvases -> the ``size x size`` pictures the image encoders were trained on
        (avae_letter_thumbnail in include/avae.h): the reference's ``get_char_img_thumbnail_helper`` (utils.py:208-258) with the
        steps its callers put in front of it, on the device and in exact integer arithmetic.

        ``frames`` is uint8, ``[N, Hf, Wf]`` or ``[N, Hf, Wf, C]`` with C = 1, 3 (RGB) or 4 (RGBA, the fourth channel ignored);
        ``channel_order='bgr'`` reads OpenCV's order.  A device tensor that is a crop or a padded view of a larger one is read in
        place.  ``threshold`` (0 .. 255) makes the grey value binary first, ``invert`` turns dark ink on a bright ground into
        bright ink; ``**letter_thumbnails.CAMERA`` is the reference's camera path (threshold 108, inverted),
        ``**letter_thumbnails.CANVAS`` its drawing pad (inverted).

        Returns a dict: ``image [N, size * size]`` float32 in [0, 1], ``box [N, 4]`` (x, y, w, h of the ink), ``window [N, 3]``
        (x, y and side of the square that was shrunk, in frame pixels; it may reach outside the frame) and ``ink [N]`` (pixels
        with ink), int32.  A frame without ink gives a picture of zeros, the whole frame as its box and ``ink = 0``."""
        t, row, frame, flags, thr, size, was_np = letter_thumbnail_args(frames, size, threshold, invert, channel_order, self.device)
        conv = self._like_input(was_np)
        return {k: conv(v) for k, v in self._letter_thumbnails(t, row, frame, flags, thr, size).items()}

    letter_thumbnails.CAMERA = THUMBNAIL_CAMERA
    letter_thumbnails.CANVAS = THUMBNAIL_CANVAS

    def frames_to_motion(self, frames, basis, image_modality=0, modality=1, **thumbnail_options):
        """From camera frames to joint trajectories without leaving the device: ``letter_thumbnails(frames,
        **thumbnail_options)``, then ``predict_motion`` with the picture as the only present modality -- bitwise those two calls.
        The thumbnail's ``size * size`` must be modality ``image_modality``'s ``n_input``.  Returns ``predict_motion``'s dict with
        ``image``, ``box``, ``window`` and ``ink`` added."""
        as_index(image_modality, "image_modality", len(self._widths))
        t, row, frame, flags, thr, size, was_np = letter_thumbnail_args(
            frames, thumbnail_options.pop("size", 28), thumbnail_options.pop("threshold", None),
            thumbnail_options.pop("invert", False), thumbnail_options.pop("channel_order", "rgb"), self.device)
        if thumbnail_options:
            raise ValueError("unknown thumbnail option(s) %s (size, threshold, invert, channel_order)"
                             % ", ".join(sorted(map(str, thumbnail_options))))
        if size * size != self._widths[image_modality]:
            raise ValueError("thumbnails of %d x %d pixels do not fit modality %d, which holds %d"
                             % (size, size, image_modality, self._widths[image_modality]))
        thumbs = self._letter_thumbnails(t, row, frame, flags, thr, size)
        X = [None] * len(self._widths)
        X[image_modality] = thumbs["image"]
        out = self.predict_motion(X, basis, modality=modality)
        out.update(thumbs)
        conv = self._like_input(was_np)
        return {k: None if v is None else conv(v) for k, v in out.items()}

    # ------------------------------------------------------------------ black-box search
    def _search_sample(self, st, R, seed, iteration, proj, x):
        """avae_search_sample on the state's Gaussians into ``x [P, R, n]`` (all problems in one call: problem_offset 0)"""
        P, n = st["mean"].shape
        A, b, G, g = proj if proj is not None else (None, None, 0, 0)
        _capi.check(self._h, self._L.avae_search_sample(
            self._h, st["mean"].data_ptr(), st["var"].data_ptr(), P, R, n, seed, iteration, 0, ptr(A), ptr(b), G, g,
            x.data_ptr(), self._stream()), "avae_search_sample")

    def _search_update(self, st, x, c, opt, avg=None, mn=None, moved=None):
        """avae_search_update of the state in place from the rollouts ``x [P, R, n]`` and their costs ``c [P, R]``"""
        P, R, n = x.shape
        _capi.check(self._h, self._L.avae_search_update(
            self._h, x.data_ptr(), c.data_ptr(), P, R, n, C.byref(opt), st["mean"].data_ptr(), st["var"].data_ptr(),
            st["n_applied"].data_ptr(), st["frozen"].data_ptr(), st["best_cost"].data_ptr(), st["best_x"].data_ptr(),
            ptr(avg), ptr(mn), ptr(moved), self._stream()), "avae_search_update")

    def search(self, cost, x0, var0, n_rollouts=10, n_iters=10, eliteness=10, weighting="PI-BB", cov_update="PI-BB",
               learning_rate=1.0, covar_bounds=(0.1,), tol=1e-6, project=None, seed=0, state=None):
        """Black-box search for P problems at once (avae_search_sample / avae_search_update in include/avae.h): the reference's
        ``GaussianCEM`` loop (pygcem.py:28-151, 154-183) with every problem's rollouts drawn, priced and refitted on the device.

        Problem p starts from N(``x0[p]``, diag(``var0``)) (``x0 [P, n]``; ``var0`` a number, ``[n]`` or ``[P, n]``); each of
        ``n_iters`` iterations draws ``n_rollouts`` candidates per problem, prices them with ``cost(candidates [rows, n],
        problem_index [rows]) -> [rows]`` and refits.  ``cost`` gets and returns device tensors and must not synchronise; it is
        called on chunks of whole problems (at most ``_motion_chunk`` rows), and the result does not depend on the chunking.  A
        NaN or Inf cost marks a candidate that could not be priced: it has no weight.  ``weighting`` 'PI-BB' (``eliteness`` = h),
        'CEM' or 'CMA-ES' (``eliteness`` = the number of candidates kept); ``cov_update`` 'PI-BB' (deviations from the old mean)
        or 'CEM' (from the new); ``covar_bounds`` None or up to three numbers (relative lower, absolute lower, absolute upper
        bound of the variances; -1 = none), as the reference's; a problem whose mean moved less than ``tol`` stops changing.
        ``project`` None or ``(A [G, g, g], b [P, n])``: every candidate's group k of g dimensions is mapped to ``A[k] x + b``.
        The draws depend on ``seed``, the iteration and the problem's index alone.

        Returns a dict of ``mean``, ``var``, ``best_x [P, n]``, ``best_cost``, ``n_applied [P]``, the histories ``avg_cost``,
        ``min_cost``, ``moved [n_iters, P]`` (NaN where a problem was not updated) and ``state``; ``search(..., state=state)``
        continues the run (``x0`` / ``var0`` are then ignored): k iterations and then m more are the bits of k + m.  The whole
        loop is enqueued without a host round trip.  NumPy in gives NumPy out (``state`` stays on the device)."""
        st, opt, R, n_iters, proj, seed, was_np = search_args(x0, var0, n_rollouts, n_iters, eliteness, weighting, cov_update,
                                                              learning_rate, covar_bounds, tol, project, seed, state, self.device)
        if not callable(cost):
            raise ValueError("cost must be callable: cost(candidates [rows, n], problem_index [rows]) -> [rows]")
        P, n = st["mean"].shape
        x = torch.empty((P, R, n), dtype=torch.float32, device=self.device)
        c = torch.empty((P, R), dtype=torch.float32, device=self.device)
        hist = {k: torch.full((n_iters, P), float("nan"), dtype=torch.float32, device=self.device)
                for k in ("avg_cost", "min_cost", "moved")}
        pidx = torch.div(torch.arange(P * R, device=self.device), R, rounding_mode="floor")
        chunk = max(1, int(self._motion_chunk) // R)
        for i in range(n_iters if P else 0):
            self._search_sample(st, R, seed, st["iteration"] + i, proj, x)
            for p0 in range(0, P, chunk):
                p1 = min(P, p0 + chunk)
                out = cost(x[p0:p1].reshape(-1, n), pidx[p0 * R:p1 * R])
                if not torch.is_tensor(out) or out.numel() != (p1 - p0) * R:
                    raise ValueError("cost must return a tensor of [%d] values, one per candidate" % ((p1 - p0) * R))
                c[p0:p1] = out.reshape(p1 - p0, R)
            self._search_update(st, x, c, opt, hist["avg_cost"][i], hist["min_cost"][i], hist["moved"][i])
        st["iteration"] += n_iters
        conv = self._like_input(was_np)
        res = {k: conv(st[k]) for k in ("mean", "var", "best_x", "best_cost", "n_applied")}
        res.update({k: conv(v) for k, v in hist.items()})
        res["state"] = st
        return res

    def refine_motion(self, target_image, basis, chain, canvas, space="latent", init=None, n_rollouts=None, n_iters=10, var0=None,
                      anchor_start=True, weights=(0.3, 10.0, 0.7), image_modality=0, modality=1, **search_options):
        """The reference's posterior refinement of a written motion (``derive_robot_motion_from_img_posterior_rl`` and
        ``..._rl_latent``, baxter_vae_assoc_writer.py:259-342) for P pictures at once: a ``search`` whose cost is
        ``writing_cost``'s against ``target_image [P, n_pixels]``.

        The start is the encoding of ``target_image`` and its decoded motion (or ``init``: ``[P, n_z]`` latents, for
        ``space='params'`` ``[P, n_params]`` parameters).  Every candidate of problem p is priced against the picture p, the
        picture's encoding and the mean pen height of p's initial motion.  ``space='latent'``: the candidates are latents,
        decoded by modality ``modality``'s decoder and drawn (``var0`` 0.01, 10 rollouts by default).  ``space='params'``: the
        candidates are the standardised parameters themselves (``var0`` ``0.001 / param_std**2``, 20 rollouts); with
        ``anchor_start`` every candidate is projected onto starting where the initial trajectory starts, joint by joint.
        ``search_options`` are ``search``'s (eliteness, weighting, cov_update, learning_rate, covar_bounds, tol, seed).

        Returns ``search``'s dict and ``params [P, n_params]`` (the refined mean motion; latent space: its decoding), ``z`` (latent
        space: the refined latent, else None), ``height [P]``, ``initial`` and ``final`` (dicts of ``cost``, ``img_l2``,
        ``height_l2``, ``latent_l2`` at the start and at ``params``: ``writing_cost``'s values at ``height``) and ``image``, the
        drawing of ``params``."""
        w = writing_cost_args(weights, image_modality, canvas, self._widths)
        R, extra = refine_motion_args(basis, chain, space, n_rollouts, modality, search_options, self._widths)
        if target_image is None:
            raise ValueError("target_image is None: the refinement needs the pictures to write")
        tg, was_np = dev_array(target_image, canvas.n_pixels, self.device)
        tg = tg.contiguous()
        P = int(tg.shape[0])
        latent = space == "latent"
        start = None if init is None else dev_dense(init, self.n_z if latent else basis.n_params, self.device, P,
                                                    "as target_image", name="init")
        mats = motion_matrices(basis, self.device)
        frames, axes = chain_matrices(chain, self.device)
        plane = canvas_args(canvas, P, None, None, self.device)[0]
        zt = self._encode(image_modality, tg)
        if latent or start is None:
            z0 = zt.clone() if start is None else start
            p0 = self._decode(modality, z0)
        else:
            p0 = start
        first = self._writing_cost(p0, mats, basis, frames, axes, plane, canvas, tg, None, zt, w, image_modality)
        h0 = first["height"]
        project = None
        if latent:
            x0, v0 = z0, 0.01 if var0 is None else var0
        else:
            x0 = p0
            v0 = var0
            if v0 is None:
                v0 = 0.001 if basis.param_std is None else 0.001 / basis.param_std ** 2
            if anchor_start:
                A, b = basis.projection([0.0], first["trajectory"][:, 0, :].reshape(P, basis.n_dof, 1).cpu().numpy())
                project = (to_device32(A, self.device), to_device32(b, self.device))

        def price(cand, pidx):
            return self._writing_cost(self._decode(modality, cand) if latent else cand, mats, basis, frames, axes, plane, canvas,
                                      tg.index_select(0, pidx), h0.index_select(0, pidx), zt.index_select(0, pidx), w,
                                      image_modality)["cost"]
        res = self.search(price, x0, v0, n_rollouts=R, n_iters=n_iters, project=project, **extra)
        params = self._decode(modality, res["mean"]) if latent else res["mean"]
        last = self._writing_cost(params, mats, basis, frames, axes, plane, canvas, tg, h0, zt, w, image_modality)
        conv = self._like_input(was_np)
        terms = ("cost", "img_l2", "height_l2", "latent_l2")
        out = {k: (v if k == "state" else conv(v)) for k, v in res.items()}
        out.update(params=conv(params), z=conv(res["mean"]) if latent else None, height=conv(h0), image=conv(last["image"]),
                   initial={k: conv(first[k]) for k in terms}, final={k: conv(last[k]) for k in terms})
        return out

    def cycle_error(self, X, basis, chain, canvas, source=0, modality=1):
        """Does the motion predicted from a picture write that picture?  ``predict_motion`` from modality ``source`` alone, the
        drawing of the predicted trajectory, and its distance from ``X[source]`` pixel by pixel (``img_l2``) and between the two
        pictures' encodings (``latent_l2``).  With ``X[modality]`` given, the same two figures for the drawing of the row's own
        recorded parameters: the floor set by the renderer and the data.  Returns ``dict(predicted=dict(img_l2, latent_l2, image),
        own=dict(...) or None)``."""
        M = len(self._widths)
        as_index(source, "source", M)
        if len(X) != M:
            raise ValueError("expected a list of %d modalities, got %d" % (M, len(X)))
        writing_cost_args((0.0, 0.0, 0.0), source, canvas, self._widths)
        only = [X[m] if m == source else None for m in range(M)]
        (ts, rows, was_np, xp, lds, p, _, _), mats = predict_motion_args(only, basis, modality, None, 0, None, None, self._widths,
                                                                        self.n_z, self.device)
        frames, axes = chain_matrices(chain, self.device)
        _same_joints(basis, chain)
        own_p = None if X[modality] is None else dev_dense(X[modality], basis.n_params, self.device, rows, "as X[%d]" % source,
                                                           name="X[%d]" % modality)
        seen = ts[source].contiguous()
        plane = canvas_args(canvas, rows, None, None, self.device)[0]
        z_seen = self._encode(source, seen)
        conv = self._like_input(was_np)

        def drawn(params):
            traj = self._motion_eval(params, mats, basis)[0]
            out = self._render(self._motion_fk(traj, frames, axes), plane, canvas, seen, None)
            lat = torch.linalg.vector_norm(self._encode(source, out["image"]) - z_seen, dim=1)
            return {"img_l2": conv(out["img_l2"]), "latent_l2": conv(lat), "image": conv(out["image"])}
        _, _, mean = self._fused_decode(xp, lds, p, rows, modality, True)
        return {"predicted": drawn(mean), "own": None if own_p is None else drawn(own_p)}

    # ------------------------------------------------------------------ inverse kinematics
    def _motion_pose(self, t, frames, axes, position=True, rotation=True, jacobian=False):
        """avae_motion_pose on device tensors: trajectories [N, T, D] -> (position [N, T, 3], rotation [N, T, 3, 3], jacobian
        [N, T, 6, D]), None for an output that is not asked for"""
        N, T, D = t.shape

        def new(want, *tail):
            return torch.empty((N, T) + tail, dtype=torch.float32, device=self.device) if want else None
        pos, rot, jac = new(position, 3), new(rotation, 3, 3), new(jacobian, 6, D)
        if N:
            _capi.check(self._h, self._L.avae_motion_pose(self._h, t.data_ptr(), N, T, D, frames.data_ptr(), axes.data_ptr(),
                                                          ptr(pos), ptr(rot), ptr(jac), self._stream()), "avae_motion_pose")
        return pos, rot, jac

    def motion_pose(self, trajectories, chain, jacobian=False):
        """Joint trajectories ``[N, T, chain.n_dof]`` -> the pen tip's pose at every point (avae_motion_pose in include/avae.h):
        a dict of ``position [N, T, 3]``, ``rotation [N, T, 3, 3]`` and, with ``jacobian=True``, the geometric Jacobian
        ``jacobian [N, T, 6, n_dof]`` (linear over angular rows, base frame; None otherwise) -- ``KinematicChain.pose`` and
        ``.jacobian`` for every row and time point in one launch.  ``position`` is ``motion_fk``'s value, not its bits."""
        t, frames, axes, want, was_np = motion_pose_args(trajectories, chain, jacobian, self.device)
        pos, rot, jac = self._motion_pose(t, frames, axes, jacobian=want)
        conv = self._like_input(was_np)
        return {"position": conv(pos), "rotation": conv(rot), "jacobian": None if jac is None else conv(jac)}

    def _motion_ik(self, p, frames, axes, seed, orient, lim, opts):
        """avae_motion_ik on device tensors, in chunks of ``_motion_chunk`` rows (rows are independent: the chunk changes no
        bit) -> dict of device tensors.  ``orient`` None, [1, 3, 3], [N, 3, 3] or 'seed': the orientation of the seed's pose."""
        N, T, D = p.shape[0], p.shape[1], seed.shape[1]
        if isinstance(orient, str):
            orient = self._motion_pose(seed.reshape(N, 1, D), frames, axes, position=False)[1].reshape(N, 3, 3)
        n_iters, tol, rot_tol, damping, max_step = opts
        traj = torch.empty((N, T, D), dtype=torch.float32, device=self.device)
        res = self._new(N, T)
        rres = None if orient is None else self._new(N, T)
        its, st = (torch.empty((N, T), dtype=torch.int32, device=self.device) for _ in range(2))
        chunk = max(1, int(self._motion_chunk))
        for r0 in range(0, N, chunk):
            n = min(chunk, N - r0)
            o = None if orient is None else (orient if orient.shape[0] == 1 else orient[r0:r0 + n])
            _capi.check(self._h, self._L.avae_motion_ik(
                self._h, p[r0:r0 + n].data_ptr(), n, T, D, frames.data_ptr(), axes.data_ptr(), seed[r0:r0 + n].data_ptr(),
                ptr(o), 0 if o is None else int(o.shape[0]), ptr(lim), n_iters, tol, rot_tol, damping, max_step,
                traj[r0:r0 + n].data_ptr(), res[r0:r0 + n].data_ptr(), None if rres is None else rres[r0:r0 + n].data_ptr(),
                its[r0:r0 + n].data_ptr(), st[r0:r0 + n].data_ptr(), self._stream()), "avae_motion_ik")
        return {"trajectory": traj, "residual": res, "rot_residual": rres, "iterations": its, "status": st, "converged": st == 0}

    def motion_ik(self, path, chain, seed, orientation=None, n_iters=20, tol=1e-5, rot_tol=1e-4, damping=0.01, max_step=0.5,
                  limits=True):
        """Pen paths ``[N, T, 3]`` -> the joint trajectories that follow them (avae_motion_ik in include/avae.h): the reference's
        ``derive_ik_trajectory`` (baxter_writer.py:84-96) for N paths at once, every point solved by damped least squares from
        the angles the previous point ended with -- the project's own definition of what PyKDL's Newton-Raphson solver does
        there, not a bit copy of it.

        ``seed`` (``[n_dof]`` or ``[N, n_dof]``) are the angles point 0 starts from.  ``orientation`` is None (position only), a
        ``[3, 3]`` rotation for every row, ``[N, 3, 3]``, or ``'seed'``: the orientation of ``chain.pose(seed)``, the reference's
        ``seed_pose[3:7]`` (a goal should lie within 90 degrees of the pose it is approached from).  A point is done when its
        position error is below ``tol`` (metres; fp32 cannot meet a ``tol`` under about 1e-6) and its orientation error
        (sin of the angle) below ``rot_tol``, or after ``n_iters`` steps; ``damping`` is the least-squares damping, ``max_step``
        the largest change of one angle in one step (radians).  ``limits``: True (the chain's own, if every joint has them), None
        or ``[n_dof, 2]``.

        Returns a dict: ``trajectory [N, T, n_dof]``, ``residual`` / ``rot_residual [N, T]`` (the errors at the returned angles;
        ``rot_residual`` None without a goal), ``iterations`` and ``status [N, T]`` (int32; 0 converged, 1 iteration cap, 2 the
        solve failed -- a Cholesky pivot that is not > 0 or a step with a non-finite angle, which is not taken: the point keeps
        its last good angles and the next point starts from them -- 3 a non-finite target or seed: NaN angles, and the next
        point starts as if that point were not there) and ``converged = status == 0``.  NumPy in gives NumPy out, device
        tensors in give device tensors out."""
        p, frames, axes, s, orient, lim, opts, was_np = motion_ik_args(path, chain, seed, orientation, n_iters, tol, rot_tol,
                                                                       damping, max_step, limits, self.device)
        conv = self._like_input(was_np)
        return {k: None if v is None else conv(v) for k, v in self._motion_ik(p, frames, axes, s, orient, lim, opts).items()}

    # ------------------------------------------------------------------ iLQR trajectory synthesis
    _track_chunk = None        # rows one avae_motion_track call takes; None: what fits the workspace bound (track_rows_per_call)

    def _motion_track(self, p, frames, axes, q0, E, lim, opts):
        """avae_motion_track on device tensors -> dict of device tensors.  Rows go in chunks of ``track_rows_per_call`` rows, so
        the workspace stays below ``_args.TRACK_WORKSPACE_BYTES`` (512 MiB) or one row's bytes (rows are independent: the chunk
        changes no bit)."""
        N, T, D = int(q0.shape[0]), int(q0.shape[1]), int(q0.shape[2])
        dt, w, R, wl, n_iters, lam0, tol = opts
        chunk, per_row = track_rows_per_call(T, D)
        if self._track_chunk is not None:
            chunk = max(1, min(chunk, int(self._track_chunk)))
        traj = torch.empty((N, T, D), dtype=torch.float32, device=self.device)
        ctrl = torch.empty((N, T - 1, D), dtype=torch.float32, device=self.device)
        c0, c1 = (torch.empty((N,), dtype=torch.float64, device=self.device) for _ in range(2))
        rm = torch.empty((N,), dtype=torch.float32, device=self.device)
        its, acc, st = (torch.empty((N,), dtype=torch.int32, device=self.device) for _ in range(3))
        ws = torch.empty((min(chunk, N) * per_row,), dtype=torch.uint8, device=self.device)
        wv = (C.c_float * 3)(*w)
        for r0 in range(0, N, chunk):
            n = min(chunk, N - r0)
            _capi.check(self._h, self._L.avae_motion_track(
                self._h, p[r0:r0 + n].data_ptr(), q0[r0:r0 + n].data_ptr(), n, T, D, frames.data_ptr(), axes.data_ptr(), dt, wv, R,
                ptr(E), ptr(lim), wl, n_iters, lam0, TRACK_FACTOR, TRACK_LAM_MIN, TRACK_LAM_MAX, tol, ws.data_ptr(), n * per_row,
                traj[r0:r0 + n].data_ptr(), ctrl[r0:r0 + n].data_ptr() if T > 1 else None, c0[r0:r0 + n].data_ptr(),
                c1[r0:r0 + n].data_ptr(), rm[r0:r0 + n].data_ptr(), its[r0:r0 + n].data_ptr(), acc[r0:r0 + n].data_ptr(),
                st[r0:r0 + n].data_ptr(), self._stream()), "avae_motion_track")
        return {"trajectory": traj, "controls": ctrl, "cost0": c0, "cost": c1, "track_rmse": rm, "iterations": its,
                "accepted": acc, "status": st}

    def motion_track(self, path, chain, seed=None, init=None, orientation=None, dt=0.01, track_weights=(10.0, 10.0, 50.0),
                     effort_weight=0.01, effort=None, limits=True, limit_weight=0.0, n_iters=25, lam0=1.0, tol=1e-6,
                     ik_options=None):
        """Pen paths ``[N, T, 3]`` -> smooth joint trajectories that follow them (avae_motion_track in include/avae.h): the
        reference's ``derive_ilqr_trajectory`` (baxter_writer.py:106-145) for N paths at once -- iLQR on a double-integrator joint
        model (``q' = q + dt v``, ``v' = v + dt u``) whose cost trades the tip's distance from the path, weighted per axis by
        ``track_weights``, against the control effort ``effort_weight |E u|^2`` -- the project's own definition of that solver, not
        a bit copy of it.

        The first guess is ``init [N, T, n_dof]`` or, with ``init=None``, ``motion_ik(path, chain, seed, orientation,
        **ik_options)``: the reference's way.  ``effort`` is None (the identity) or a constant ``[n_dof, n_dof]`` matrix E, for
        example the square root of the arm's inertia at the seed pose (the chain carries no masses).  ``limits`` (True: the
        chain's own, None or ``[n_dof, 2]``) enter as a quadratic penalty ``limit_weight`` on what an angle lies outside them,
        and not at all at ``limit_weight=0``.  A try solves the Riccati recursion at the damping ``lam`` (``lam0`` at first, a
        tenth after an accepted try, tenfold after a rejected one, between 1e-6 and 1e6) and takes the full step if it lowers the
        cost; a row ends after ``n_iters`` tries, when an accepted try gains less than ``tol`` of the cost, or when ``lam`` passes
        1e6.  Rows go to the device in chunks whose workspace stays below 512 MiB (or one row's).

        Returns a dict: ``trajectory [N, T, n_dof]``, ``controls [N, T - 1, n_dof]`` (joint accelerations), ``cost0`` and ``cost
        [N]`` (float64; of the first guess's rollout and of the result), ``track_rmse [N]`` (metres, unweighted), ``iterations``
        and ``accepted [N]`` (tries made and taken) and ``status [N]`` (int32; 0 converged, 1 ``n_iters`` tries made, 2 no try
        was ever accepted, 3 a non-finite path point, first guess or limit: NaN outputs).  NumPy in gives NumPy out, device
        tensors in give device tensors out."""
        p, frames, axes, q0, E, lim, opts, was_np = motion_track_args(path, chain, init, dt, track_weights, effort_weight, effort,
                                                                      limits, limit_weight, n_iters, lam0, tol, self.device)
        if q0 is None:
            extra = set(ik_options or {}) - {"n_iters", "tol", "rot_tol", "damping", "max_step", "limits"}
            if extra:
                raise ValueError("unknown ik_options %s" % ", ".join(sorted(map(str, extra))))
            ik = dict(dict(n_iters=20, tol=1e-5, rot_tol=1e-4, damping=0.01, max_step=0.5, limits=True), **(ik_options or {}))
            a = motion_ik_args(p, chain, seed, orientation, ik["n_iters"], ik["tol"], ik["rot_tol"], ik["damping"], ik["max_step"],
                               ik["limits"], self.device)
            q0 = self._motion_ik(*a[:7])["trajectory"]
        elif seed is not None or orientation is not None or ik_options is not None:
            raise ValueError("seed, orientation and ik_options belong to the first guess motion_ik makes: leave them out with init")
        conv = self._like_input(was_np)
        return {k: conv(v) for k, v in self._motion_track(p, frames, axes, q0, E, lim, opts).items()}

    def _smoothed(self, p, chain, traj, tr):
        """``_motion_track`` from the trajectory ``traj`` with the options dict ``tr`` (``check_solver``'s)"""
        p, frames, axes, q0, E, lim, opts, _ = motion_track_args(p, chain, traj, tr["dt"], tr["track_weights"], tr["effort_weight"],
                                                                 tr["effort"], tr["limits"], tr["limit_weight"], tr["n_iters"],
                                                                 tr["lam0"], tr["tol"], self.device)
        return self._motion_track(p, frames, axes, q0, E, lim, opts)

    def strokes_to_motion(self, strokes, basis, chain, canvas, center, seed, height=0.0, solver="ik", track_options=None,
                          **ik_options):
        """The reference's data pipeline (``build_ik_joint_traj_for_chars`` and ``build_fa_for_joint_trajs``,
        baxter_writer.py:147-196) for N strokes at once: ``strokes [N, T, 2]`` in the canvas' plane units are lifted around
        ``center`` at ``height`` above the paper (``canvas.lift``), followed by the arm (``motion_ik`` from ``seed`` with
        ``ik_options``), fitted (``motion_fit`` with ``basis``, whose ``n_points`` must be T) and drawn (``render_strokes``).
        With ``solver='ilqr'`` the inverse-kinematics solution is the first guess of ``motion_track`` (``track_options``: a dict
        of its dt, track_weights, effort_weight, effort, limits, limit_weight, n_iters, lam0, tol), the reference's
        ``build_ilqr_joint_traj_for_chars`` (baxter_writer.py:166-184), and the smoothed motion is what is fitted.

        Returns a dict: ``path [N, T, 3]``, ``trajectory [N, T, n_dof]``, ``params [N, n_params]`` (a joint-modality row),
        ``image [N, n_pixels]`` (the image-modality row), ``converged [N]`` (every point of the row, of ``motion_ik``),
        ``fit_rmse [N, n_dof]`` (``motion_eval`` of the fitted parameters against the trajectory) and ``tip_error [N]`` (the
        worst distance of the pen tip of the fitted motion from the path: what approximator and solver lose together); under
        ``'ilqr'`` also ``track_status`` and ``track_cost [N]``.  Every piece is bitwise what the separate calls give."""
        tr = check_solver(solver, track_options)
        (p, frames, axes, s, orient, lim, opts), was_np = strokes_to_motion_args(strokes, basis, chain, canvas, center, seed, height,
                                                                                 ik_options, self.device)
        ik = self._motion_ik(p, frames, axes, s, orient, lim, opts)
        sm = None if tr is None else self._smoothed(p, chain, ik["trajectory"], tr)
        t, pinv, sc, sh, _ = motion_fit_args(ik["trajectory"] if sm is None else sm["trajectory"], basis, self.device)
        params = self._motion_fit(t, pinv, sc, sh, basis)
        ev, _, rmse, _ = self._motion_eval(params, motion_matrices(basis, self.device), basis, ref=t)
        tip = torch.linalg.vector_norm(self._motion_fk(ev, frames, axes) - p, dim=2).amax(1)
        plane = canvas_args(canvas, int(p.shape[0]), None, None, self.device)[0]
        image = self._render(p, plane, canvas, None, None)["image"]
        conv = self._like_input(was_np)
        out = {"path": conv(p), "trajectory": conv(t), "params": conv(params), "image": conv(image),
               "converged": conv(ik["converged"].all(1)), "fit_rmse": conv(rmse), "tip_error": conv(tip)}
        if sm is not None:
            out.update(track_status=conv(sm["status"]), track_cost=conv(sm["cost"]))
        return out

    def refine_pen_path(self, target_image, basis, chain, canvas, init=None, n_rollouts=50, n_iters=20, var0=1e-5,
                        anchor_start=True, seed_angles=None, image_modality=0, modality=1, ik_n_iters=20, solver="ik",
                        track_options=None, **options):
        """The reference's Cartesian refinement (``derive_robot_motion_from_img_posterior_rl_cartesian``,
        baxter_vae_assoc_writer.py:182-257) for P pictures at once: a ``search`` over the pen path's own approximator parameters
        and the way back to joint space.

        The start is the motion decoded from the encoding of ``target_image [P, n_pixels]`` (or ``init``: ``[P, n_params]``
        standardised parameters), evaluated and run through ``motion_fk``.  The two in-plane coordinates of that path are fitted
        with a two-joint basis of ``basis.n_basis`` features (``motion_fit``); with ``anchor_start`` every candidate is projected
        onto starting where that path starts.  The candidates (``2 (n_basis + 1)`` numbers, ``var0`` their first variance) are
        evaluated, put back at the initial path's own height point by point, drawn and priced by ``img_l2`` against the picture
        -- the image term of the reference's ``cost_robot_cart_motion_img`` alone.  The refined mean is evaluated the same way,
        followed by ``motion_ik`` (seeded with the initial motion's first angles, or ``seed_angles [P, n_dof]``) and fitted with
        ``basis``.  ``n_iters`` counts the search's iterations, ``ik_n_iters`` is the solver's cap.  ``options`` are
        ``motion_ik``'s (orientation, tol, rot_tol, damping, max_step, limits) and ``search``'s (eliteness, weighting, cov_update,
        learning_rate, covar_bounds, seed, and ``tol_search`` for its ``tol``: ``tol`` is the solver's).  Between the first draw
        and the last fit there is no host round trip.

        Returns ``search``'s dict and ``path [P, T, 3]`` (the refined pen path), ``trajectory [P, T, n_dof]``, ``params
        [P, n_params]`` (bitwise ``motion_fit(motion_ik(path, ...)["trajectory"], basis)``), ``converged [P]``, ``initial`` and
        ``final`` (dicts of ``img_l2 [P]`` of the initial path and of ``path``) and ``image``, the drawing of ``path``.  With
        ``solver='ilqr'`` the way back to joint space goes on through ``motion_track`` (``track_options``: a dict of its options)
        from the inverse-kinematics solution: ``trajectory`` and ``params`` are those of the smoothed motion, and the dict also
        holds ``track_status`` and ``track_cost [P]``."""
        tr = check_solver(solver, track_options)
        ik, search_options = refine_pen_path_args(basis, chain, canvas, n_rollouts, dict(options, n_iters=ik_n_iters), self._widths,
                                                  image_modality, modality)
        if target_image is None:
            raise ValueError("target_image is None: the refinement needs the pictures to write")
        tg, was_np = dev_array(target_image, canvas.n_pixels, self.device)
        tg = tg.contiguous()
        P, T = int(tg.shape[0]), basis.n_points
        if init is None:
            p0 = self._decode(modality, self._encode(image_modality, tg))
        else:
            p0 = dev_dense(init, basis.n_params, self.device, P, "as target_image", name="init")
        mats = motion_matrices(basis, self.device)
        frames, axes = chain_matrices(chain, self.device)
        plane = canvas_args(canvas, P, None, None, self.device)[0]
        back = to_device32(np.linalg.inv(canvas.plane).T, self.device)
        traj0 = self._motion_eval(p0, mats, basis)[0]
        path0 = self._motion_fk(traj0, frames, axes)
        uvn = path0 @ plane.T                                                       # [P, T, 3]: in-plane u, v and the height n
        flat = MotionBasis(kind=basis.kind, n_basis=basis.n_basis, n_dof=2, n_points=T, normalize=basis.normalize)
        fmats = motion_matrices(flat, self.device)
        uv0, n0 = uvn[:, :, :2].contiguous(), uvn[:, :, 2:].contiguous()
        x0 = self._motion_fit(*motion_fit_args(uv0, flat, self.device)[:4], flat)
        project = None
        if anchor_start and P:
            A, b = flat.projection([0.0], uv0[:, 0, :].reshape(P, 2, 1).cpu().numpy())
            project = (to_device32(A, self.device), to_device32(b, self.device))
        seed = traj0[:, 0, :] if seed_angles is None else seed_angles

        def pen_path(x, height):
            return (torch.cat([self._motion_eval(x, fmats, flat)[0], height], dim=2) @ back).contiguous()

        def price(cand, pidx):
            return self._render(pen_path(cand, n0.index_select(0, pidx)), plane, canvas, tg.index_select(0, pidx), None)["img_l2"]
        first = self._render(path0, plane, canvas, tg, None)
        res = self.search(price, x0, var0, n_rollouts=n_rollouts, n_iters=n_iters, project=project, **search_options)
        path = pen_path(res["mean"], n0)
        p, frames, axes, s, orient, lim, opts, _ = motion_ik_args(path, chain, seed, ik["orientation"], ik["n_iters"], ik["tol"],
                                                                  ik["rot_tol"], ik["damping"], ik["max_step"], ik["limits"],
                                                                  self.device)
        sol = self._motion_ik(p, frames, axes, s, orient, lim, opts)
        sm = None if tr is None else self._smoothed(p, chain, sol["trajectory"], tr)
        if sm is not None:
            sol = dict(sol, trajectory=sm["trajectory"])
        params = self._motion_fit(*motion_fit_args(sol["trajectory"], basis, self.device)[:4], basis)
        last = self._render(path, plane, canvas, tg, None)
        conv = self._like_input(was_np)
        out = {k: (v if k == "state" else conv(v)) for k, v in res.items()}
        out.update(path=conv(path), trajectory=conv(sol["trajectory"]), params=conv(params),
                   converged=conv(sol["converged"].all(1)), image=conv(last["image"]),
                   initial={"img_l2": conv(first["img_l2"])}, final={"img_l2": conv(last["img_l2"])})
        if sm is not None:
            out.update(track_status=conv(sm["status"]), track_cost=conv(sm["cost"]))
        return out

    # ------------------------------------------------------------------ sigma-lognormal strokes
    _lognormal_chunk = 16384   # rows (eval, fit) or rows x samples (sample) one launch takes

    def _lognormal_eval(self, p, cnt, st, T, dt, velocity=True):
        """avae_lognormal_eval on device tensors, in chunks of rows (rows are independent: the chunk changes no bit) ->
        (path [N, T, 2], velocity [N, T, 2] or None)"""
        N, Cn = int(p.shape[0]), int(p.shape[1])
        path = torch.empty((N, T, 2), dtype=torch.float32, device=self.device)
        vel = torch.empty((N, T, 2), dtype=torch.float32, device=self.device) if velocity else None
        chunk = max(1, int(self._lognormal_chunk))
        for r0 in range(0, N, chunk):
            n = min(chunk, N - r0)
            _capi.check(self._h, self._L.avae_lognormal_eval(
                self._h, p[r0:r0 + n].data_ptr(), cnt[r0:r0 + n].data_ptr(), st[r0:r0 + n].data_ptr(), n, Cn, T, dt,
                path[r0:r0 + n].data_ptr(), None if vel is None else vel[r0:r0 + n].data_ptr(), self._stream()),
                "avae_lognormal_eval")
        return path, vel

    def lognormal_eval(self, params, n_points, count=None, start=None, dt=None):
        """Sigma-lognormal components ``params [N, C, 6]`` (``D, t0, mu, sigma, theta_s, theta_e`` per component, C <= 16) -> the
        strokes they draw (avae_lognormal_eval in include/avae.h; the reference's ``rxzero_traj_eval``, pytrajkin_rxzero.py:241-292,
        for N strokes at once).  Row n uses its first ``count[n]`` components (default: all C) and starts from ``start`` (``[2]``,
        ``[N, 2]``; default the origin); the ``n_points`` (<= 1024) time points are ``k * dt`` (``dt`` defaults to
        ``1 / (n_points - 1)``).  Returns a dict: ``path [N, n_points, 2]`` and ``velocity [N, n_points, 2]``.  A row with a
        non-finite parameter or start is NaN.  NumPy in gives NumPy out, device tensors in give device tensors out."""
        p, cnt, st, T, dt32, was_np = lognormal_eval_args(params, n_points, count, start, dt, self.device)
        path, vel = self._lognormal_eval(p, cnt, st, T, dt32)
        conv = self._like_input(was_np)
        return {"path": conv(path), "velocity": conv(vel)}

    def _lognormal_fit(self, s, p, cnt, st, dt, opts, fr, lo, hi):
        """avae_lognormal_fit on device tensors, in chunks of rows -> dict of device tensors"""
        N, T, Cn = int(s.shape[0]), int(s.shape[1]), int(p.shape[1])
        n_iters, wp, wv, tol = opts
        out = torch.empty((N, Cn, 6), dtype=torch.float32, device=self.device)
        l0, l1 = (torch.empty((N,), dtype=torch.float64, device=self.device) for _ in range(2))
        its, acc, stt = (torch.empty((N,), dtype=torch.int32, device=self.device) for _ in range(3))
        per_row = fr is not None and fr.dim() == 3
        chunk = max(1, int(self._lognormal_chunk))
        for r0 in range(0, N, chunk):
            n = min(chunk, N - r0)
            f = None if fr is None else (fr[r0:r0 + n] if per_row else fr)
            _capi.check(self._h, self._L.avae_lognormal_fit(
                self._h, s[r0:r0 + n].data_ptr(), p[r0:r0 + n].data_ptr(), cnt[r0:r0 + n].data_ptr(), st[r0:r0 + n].data_ptr(),
                n, Cn, T, dt, n_iters, wp, wv, tol, ptr(f), 1 if per_row else 0, ptr(lo), ptr(hi),
                out[r0:r0 + n].data_ptr(), l0[r0:r0 + n].data_ptr(), l1[r0:r0 + n].data_ptr(), its[r0:r0 + n].data_ptr(),
                acc[r0:r0 + n].data_ptr(), stt[r0:r0 + n].data_ptr(), self._stream()), "avae_lognormal_fit")
        return {"params": out, "count": cnt, "loss0": l0, "loss": l1, "iterations": its, "accepted": acc, "status": stt}

    def lognormal_fit(self, strokes, init=None, count=None, start=None, dt=None, max_components=8, n_iters=40,
                      weights=(1.0, 1e-3), free=None, bounds=None, tol=1e-9):
        """Fits sigma-lognormal components to ``strokes [N, T, 2]`` by Levenberg-Marquardt, every row's whole loop inside one
        launch (avae_lognormal_fit in include/avae.h): the project's own stand-in for the reference's ``rxzero_train``, not a copy
        of its three-stage optimiser.

        ``init [N, C, 6]`` with ``count [N]`` are the components to start from.  ``init=None`` runs ``lognormal_initial_guess``
        (at most ``max_components`` speed peaks per stroke) on the host: that is the call's one host read of the strokes.
        ``start`` defaults to each stroke's first point, ``dt`` to ``1 / (T - 1)``.  The loss is ``weights[0]`` times the squared
        position error plus ``weights[1]`` times the squared velocity error.  ``free`` (``[6]`` or ``[N, C, 6]``, nonzero = free)
        takes parameters out of the fit; ``bounds = (lo, hi)``, each None or ``[6]``, clips a step (``sigma`` always stays in
        [1e-3, 3]).  A row stops after ``n_iters`` tries, or when an accepted step lowers the loss by less than ``tol`` times it.

        Returns a dict: ``params [N, C, 6]``, ``count [N]``, ``loss0`` and ``loss [N]`` (float64, at the start and the end),
        ``iterations``, ``accepted``, ``status [N]`` (int32; 0 converged -- by ``tol``, or 8 tries in a row rejected after an
        accepted step: the floor of float32 --, 1 iteration cap, 2 no step accepted at all in 8 tries: the row cannot improve, 3 a non-finite stroke, start or initial parameter: NaN outputs), ``path [N, T, 2]`` (``lognormal_eval`` of the
        fitted components) and ``rmse [N]`` (root mean squared distance of ``path`` from the stroke)."""
        s, p, cnt, st, dt32, opts, fr, lo, hi, was_np = lognormal_fit_args(strokes, init, count, start, dt, max_components, n_iters,
                                                                             weights, free, bounds, tol, self.device)
        out = self._lognormal_fit(s, p, cnt, st, dt32, opts, fr, lo, hi)
        path = self._lognormal_eval(out["params"], cnt, st, int(s.shape[1]), dt32, velocity=False)[0]
        out["path"] = path
        out["rmse"] = torch.sqrt(((path - s) ** 2).sum(dim=2).mean(dim=1))
        conv = self._like_input(was_np)
        return {k: conv(v) for k, v in out.items()}

    def _lognormal_sample(self, p, cnt, st, T, dt, S, seed, amplitude, angle, straightness, shift_mean, want_params=True):
        """avae_lognormal_sample on device tensors, in chunks of rows whose first row is the call's row_offset (the chunk changes
        no bit) -> (strokes [N, S, T, 2], perturbed [N, S, C, 6] or None)"""
        N, Cn = int(p.shape[0]), int(p.shape[1])
        out = torch.empty((N, S, T, 2), dtype=torch.float32, device=self.device)
        pert = torch.empty((N, S, Cn, 6), dtype=torch.float32, device=self.device) if want_params else None
        chunk = max(1, int(self._lognormal_chunk) // S)
        for r0 in range(0, N, chunk):
            n = min(chunk, N - r0)
            _capi.check(self._h, self._L.avae_lognormal_sample(
                self._h, p[r0:r0 + n].data_ptr(), cnt[r0:r0 + n].data_ptr(), st[r0:r0 + n].data_ptr(), n, S, Cn, T, dt, seed, r0,
                amplitude, angle, straightness, 1 if shift_mean else 0, out[r0:r0 + n].data_ptr(),
                None if pert is None else pert[r0:r0 + n].data_ptr(), self._stream()), "avae_lognormal_sample")
        return out, pert

    def lognormal_augment(self, strokes=None, params=None, count=None, n_samples=10, seed=0, amplitude=0.2, angle=np.pi / 9,
                          straightness=0.1, shift_mean=True, start=None, dt=None, n_points=None, **fit_options):
        """The reference's ``extend_data_with_lognormal_sampling_helper`` (utils.py:331-359) for N strokes at once: every
        component's amplitude, start angle and straightness are perturbed by a third of a normal draw times ``amplitude`` (of
        ``D``), ``angle`` (radians, both angles) and ``straightness`` (of ``theta_e - theta_s``), and the stroke is evaluated
        again -- ``n_samples`` times per row, perturbation and evaluation fused in one launch (avae_lognormal_sample in
        include/avae.h).  With ``shift_mean`` every sample has its own mean point subtracted.

        Given ``strokes [N, T, 2]`` the components are fitted first (``lognormal_fit`` with ``fit_options``: init, max_components,
        n_iters, weights, free, bounds, tol); given ``params [N, C, 6]`` (with ``count``, ``n_points`` and optionally ``start``,
        ``dt``) they are perturbed as they are.  The draws depend on ``seed`` and the row's index alone.

        Returns a dict: ``strokes [N, n_samples, T, 2]``, ``params [N, C, 6]`` and ``count [N]`` (the components perturbed),
        ``perturbed [N, n_samples, C, 6]`` and ``status [N]`` (the fit's; zeros without one).  A row whose fit ended with status 2
        or 3 returns its samples as NaN (the reference drops such a letter with a message): ``status`` names it."""
        way = lognormal_augment_args(strokes, params, count, start, dt, n_points, self.device)
        S, seed, amplitude, angle, straightness = lognormal_sample_options(n_samples, seed, amplitude, angle, straightness)
        if way == "strokes":
            extra = set(fit_options) - {"init", "max_components", "n_iters", "weights", "free", "bounds", "tol"}
            if extra:
                raise ValueError("unknown option(s) %s (lognormal_fit takes init, max_components, n_iters, weights, free, bounds, "
                                 "tol)" % ", ".join(sorted(map(str, extra))))
            s, p0, cnt, st, dt32, opts, fr, lo, hi, was_np = lognormal_fit_args(
                strokes, fit_options.get("init"), count, start, dt, fit_options.get("max_components", 8),
                fit_options.get("n_iters", 40), fit_options.get("weights", (1.0, 1e-3)), fit_options.get("free"),
                fit_options.get("bounds"), fit_options.get("tol", 1e-9), self.device)
            fit = self._lognormal_fit(s, p0, cnt, st, dt32, opts, fr, lo, hi)
            p, status, T = fit["params"], fit["status"], int(s.shape[1])
        else:
            if fit_options:
                raise ValueError("fit options (%s) need strokes to fit" % ", ".join(sorted(map(str, fit_options))))
            p, cnt, st, T, dt32, was_np = lognormal_eval_args(params, n_points, count, start, dt, self.device)
            status = torch.zeros((int(p.shape[0]),), dtype=torch.int32, device=self.device)
        out, pert = self._lognormal_sample(p, cnt, st, T, dt32, S, seed, amplitude, angle, straightness, bool(shift_mean))
        failed = status >= 2
        out = torch.where(failed[:, None, None, None], torch.full_like(out, float("nan")), out)
        conv = self._like_input(was_np)
        return {"strokes": conv(out), "params": conv(p), "count": conv(cnt), "perturbed": conv(pert), "status": conv(status)}

    def save_model(self, fname=None):
        """reference vae_assoc.py:427-435 (default name: timestamp + batch size)."""
        if fname is None:
            ts = time.time()
            ckpt_fname = 'vae_assoc_' + datetime.datetime.fromtimestamp(ts).strftime('%Y_%m_%d_%H_%M_%S') \
                + '_batchsize_{}.ckpt'.format(self.batch_size)
        else:
            ckpt_fname = fname
        print('Saving model to {}...'.format(ckpt_fname))
        _capi.check(self._h, self._L.avae_save(self._h, os.fsencode(ckpt_fname)), "avae_save")
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
