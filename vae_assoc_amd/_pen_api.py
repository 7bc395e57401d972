"""The pen and motion methods of ``AssocVariationalAutoEncoder`` (DESIGN.md sections 23-30): motion decoding, pen-path
kinematics and stroke rendering, letter thumbnails, black-box search, inverse kinematics, iLQR tracking and sigma-lognormal
strokes.

``PenAPI`` is a mixin of ``vae_assoc.AssocVariationalAutoEncoder``: its methods reach the model through ``self`` alone
(``_encode``, ``_decode``, ``_fused_decode``, ``_call``, ``_out``, ``_like_input``), and this module imports nothing from
``vae_assoc``.  They are what the reference's writer scripts do around the model, for many rows at once.

The gradients of the writing chain stand behind the class as functions of a model: ``render_strokes_vjp``,
``motion_fk_vjp``, ``motion_eval_vjp``, ``rows_adam``, ``writing_cost_grad``, ``descend_motion``; so do the rigid-body dynamics
of the arm (section 32): ``motion_dynamics``, ``motion_effort``."""
import ctypes as C

import numpy as np
import torch

from ._args import (THUMBNAIL_CAMERA, THUMBNAIL_CANVAS, TRACK_FACTOR, TRACK_LAM_MAX, TRACK_LAM_MIN, _same_joints,
                    adam_options, canvas_args, chain_matrices, check_solver, cost_weights, descend_motion_args,
                    descent_state, draw_args, letter_thumbnail_args, lognormal_augment_args, lognormal_eval_args,
                    lognormal_fit_args, lognormal_sample_options, motion_dynamics_args, motion_effort_args, motion_eval_args,
                    motion_eval_vjp_args, motion_fit_args,
                    motion_fk_args, motion_fk_vjp_args, motion_ik_args, motion_matrices, motion_moments_args,
                    motion_pose_args, motion_track_args, predict_motion_args, refine_motion_args, refine_pen_path_args,
                    render_args, render_vjp_args, rows_adam_args, search_args, strokes_to_motion_args, track_rows_per_call,
                    writing_cost_args)
from ._marshal import as_index, dev_array, dev_dense, ptr, row_chunks, to_device32
from .motion import MotionBasis


class PenAPI(object):
    # ------------------------------------------------------------------ motion decoding
    _motion_chunk = 16384      # decoded rows (input rows x samples) predict_motion holds at a time

    def _motion_eval(self, p, mats, basis, ref=None, refp=None):
        """avae_motion_eval on device tensors -> (trajectory [N, T, D], saturated [N, D] int32, rmse, max_abs [N, D] or None)"""
        N, T, D = p.shape[0], basis.n_points, basis.n_dof
        traj = self._out((N, T, D))
        sat = self._out((N, D), torch.int32)
        has_ref = ref is not None or refp is not None
        rmse, mx = (self._out((N, D)), self._out((N, D))) if has_ref else (None, None)
        if N:
            self._call("avae_motion_eval", p.data_ptr(), N, D, basis.n_kb, T, mats["phi"].data_ptr(), ptr(mats["scale"]),
                       ptr(mats["shift"]), ptr(mats["limits"]), ptr(mats["gain"]), ptr(mats["target"]), mats["nc"], ptr(ref),
                       ptr(refp), traj.data_ptr(), sat.data_ptr(), ptr(rmse), ptr(mx))
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
        return {"trajectory": conv(traj), "saturated": conv(sat), "rmse": conv(rmse), "max_abs": conv(mx)}

    def motion_fit(self, trajectories, basis):
        """Joint trajectories ``[N, T, n_dof]`` -> standardised parameters ``[N, basis.n_params]`` (avae_motion_fit): the
        least-squares fit of the basis at ``linspace(0, 1, T)`` with the reference's truncated pseudo-inverse, per joint, then
        ``(theta - param_mean) / param_std`` (baxter_writer.py:77-82, 193).  T is the input's own."""
        t, pinv, sc, sh, was_np = motion_fit_args(trajectories, basis, self.device)
        return self._like_input(was_np)(self._motion_fit(t, pinv, sc, sh, basis))

    def _motion_fit(self, t, pinv, sc, sh, basis):
        """avae_motion_fit on device tensors: trajectories [N, T, D] -> standardised parameters [N, P]"""
        N, T = t.shape[0], t.shape[1]
        out = self._out((N, basis.n_params))
        if N:
            self._call("avae_motion_fit", t.data_ptr(), N, basis.n_dof, basis.n_kb, T, pinv.data_ptr(), ptr(sc), ptr(sh),
                       out.data_ptr())
        return out

    def _motion_moments(self, s, N, S, mats, basis, mean, var, frac):
        """avae_motion_moments on N rows of S dense samples at ``s`` into (slices of) the outputs"""
        self._call("avae_motion_moments", s.data_ptr(), N, S, basis.n_dof, basis.n_kb, basis.n_points, mats["phi"].data_ptr(),
                   ptr(mats["scale"]), ptr(mats["shift"]), ptr(mats["limits"]), ptr(mats["gain"]), ptr(mats["target"]), mats["nc"],
                   mean.data_ptr(), ptr(var), ptr(frac))

    def motion_moments(self, samples, basis, anchor=None):
        """Per-point mean and population variance of the trajectories of S parameter samples per row (avae_motion_moments):
        ``samples`` is ``[N, S, basis.n_params]``, every sample evaluated as by ``motion_eval`` (clamp included) and folded into
        running moments on the device; the ``N S n_points n_dof`` trajectory values are never stored.  Returns a dict: ``mean`` and
        ``var [N, n_points, n_dof]`` and ``saturated_frac [N, n_dof]``, the share of clamped points over samples and time."""
        s, mats, was_np = motion_moments_args(samples, basis, anchor, self.device)
        N, S = s.shape[0], s.shape[1]
        shape = (N, basis.n_points, basis.n_dof)
        mean, var = (self._out(shape) for _ in range(2))
        frac = self._out((N, basis.n_dof))
        if N:
            self._motion_moments(s, N, S, mats, basis, mean, var, frac)
        conv = self._like_input(was_np)
        return {"mean": conv(mean), "var": conv(var), "saturated_frac": conv(frac)}

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
        traj, var = (self._out(shape) for _ in range(2))
        frac = self._out((rows, basis.n_dof))
        if e is None:
            e = torch.randn((rows, S, self.n_z), dtype=torch.float32, device=self.device)
        sd = torch.exp(0.5 * lv)
        chunk = max(1, int(self._motion_chunk) // S)
        dec = self._out((min(chunk, rows) * S, basis.n_params))
        target = mats["target"]
        for r0, n, _ in row_chunks(rows, chunk):
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
        path = self._out((N, T, 3))
        if N:
            self._call("avae_motion_fk", t.data_ptr(), N, T, D, frames.data_ptr(), axes.data_ptr(), path.data_ptr())
        return path

    def _render(self, p, plane, canvas, target, height):
        """avae_stroke_render on device tensors -> dict of device tensors (``img_l2`` / ``height_l2`` None without their input)"""
        N, T, H = p.shape[0], p.shape[1], canvas.size
        image, window = self._out((N, H * H)), self._out((N, 3))
        l2 = None if target is None else self._out(N)
        hl2 = None if height is None else self._out(N)
        if N:
            self._call("avae_stroke_render", p.data_ptr(), N, T, plane.data_ptr(), canvas.half_width, canvas.margin, H,
                       canvas.supersample, ptr(target), ptr(height), image.data_ptr(), window.data_ptr(), ptr(l2), ptr(hl2))
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
        return {k: conv(v) for k, v in self._render(p, plane, canvas, tg, hg).items()}

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
        return {k: conv(v) for k, v in out.items()}

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
        image = self._out((N, size * size))
        box, window, ink = (self._out(s, torch.int32) for s in ((N, 4), (N, 3), (N,)))
        if N:
            need = C.c_size_t(0)
            if self._L.avae_letter_thumbnail_plan(N, Hf, Wf, None, C.byref(need)) != 0:
                raise RuntimeError("avae_letter_thumbnail_plan failed: %s" % self._L.avae_last_error(None).decode("utf-8", "replace"))
            ws = self._out(need.value, torch.uint8)
            self._call("avae_letter_thumbnail", t.data_ptr(), N, Hf, Wf, Cn, row, frame, flags, thr, size, ws.data_ptr(), need.value,
                       image.data_ptr(), box.data_ptr(), window.data_ptr(), ink.data_ptr())
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
        return {k: conv(v) for k, v in out.items()}

    # ------------------------------------------------------------------ black-box search
    def _search_sample(self, st, R, seed, iteration, proj, x):
        """avae_search_sample on the state's Gaussians into ``x [P, R, n]`` (all problems in one call: problem_offset 0)"""
        P, n = st["mean"].shape
        A, b, G, g = proj if proj is not None else (None, None, 0, 0)
        self._call("avae_search_sample", st["mean"].data_ptr(), st["var"].data_ptr(), P, R, n, seed, iteration, 0, ptr(A), ptr(b),
                   G, g, x.data_ptr())

    def _search_update(self, st, x, c, opt, avg=None, mn=None, moved=None):
        """avae_search_update of the state in place from the rollouts ``x [P, R, n]`` and their costs ``c [P, R]``"""
        P, R, n = x.shape
        self._call("avae_search_update", x.data_ptr(), c.data_ptr(), P, R, n, C.byref(opt), st["mean"].data_ptr(),
                   st["var"].data_ptr(), st["n_applied"].data_ptr(), st["frozen"].data_ptr(), st["best_cost"].data_ptr(),
                   st["best_x"].data_ptr(), ptr(avg), ptr(mn), ptr(moved))

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
        x, c = self._out((P, R, n)), self._out((P, R))
        hist = {k: torch.full((n_iters, P), float("nan"), dtype=torch.float32, device=self.device)
                for k in ("avg_cost", "min_cost", "moved")}
        pidx = torch.div(torch.arange(P * R, device=self.device), R, rounding_mode="floor")
        for i in range(n_iters if P else 0):
            self._search_sample(st, R, seed, st["iteration"] + i, proj, x)
            for p0, k, _ in row_chunks(P, int(self._motion_chunk) // R):
                p1 = p0 + k
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
            return self._out((N, T) + tail) if want else None
        pos, rot, jac = new(position, 3), new(rotation, 3, 3), new(jacobian, 6, D)
        if N:
            self._call("avae_motion_pose", t.data_ptr(), N, T, D, frames.data_ptr(), axes.data_ptr(), ptr(pos), ptr(rot), ptr(jac))
        return pos, rot, jac

    def motion_pose(self, trajectories, chain, jacobian=False):
        """Joint trajectories ``[N, T, chain.n_dof]`` -> the pen tip's pose at every point (avae_motion_pose in include/avae.h):
        a dict of ``position [N, T, 3]``, ``rotation [N, T, 3, 3]`` and, with ``jacobian=True``, the geometric Jacobian
        ``jacobian [N, T, 6, n_dof]`` (linear over angular rows, base frame; None otherwise) -- ``KinematicChain.pose`` and
        ``.jacobian`` for every row and time point in one launch.  ``position`` is ``motion_fk``'s value, not its bits."""
        t, frames, axes, want, was_np = motion_pose_args(trajectories, chain, jacobian, self.device)
        pos, rot, jac = self._motion_pose(t, frames, axes, jacobian=want)
        conv = self._like_input(was_np)
        return {"position": conv(pos), "rotation": conv(rot), "jacobian": conv(jac)}

    def _motion_ik(self, p, frames, axes, seed, orient, lim, opts):
        """avae_motion_ik on device tensors, in chunks of ``_motion_chunk`` rows (rows are independent: the chunk changes no
        bit) -> dict of device tensors.  ``orient`` None, [1, 3, 3], [N, 3, 3] or 'seed': the orientation of the seed's pose."""
        N, T, D = p.shape[0], p.shape[1], seed.shape[1]
        if isinstance(orient, str):
            orient = self._motion_pose(seed.reshape(N, 1, D), frames, axes, position=False)[1].reshape(N, 3, 3)
        n_iters, tol, rot_tol, damping, max_step = opts
        traj = self._out((N, T, D))
        res = self._out((N, T))
        rres = None if orient is None else self._out((N, T))
        its, st = (self._out((N, T), torch.int32) for _ in range(2))
        for r0, n, at in row_chunks(N, self._motion_chunk):
            o = None if orient is None else (orient if orient.shape[0] == 1 else orient[r0:r0 + n])
            self._call("avae_motion_ik", at(p), n, T, D, frames.data_ptr(), axes.data_ptr(), at(seed), ptr(o),
                       0 if o is None else int(o.shape[0]), ptr(lim), n_iters, tol, rot_tol, damping, max_step, at(traj), at(res),
                       at(rres), at(its), at(st))
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
        return {k: conv(v) for k, v in self._motion_ik(p, frames, axes, s, orient, lim, opts).items()}

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
        traj = self._out((N, T, D))
        ctrl = self._out((N, T - 1, D))
        c0, c1 = (self._out((N,), torch.float64) for _ in range(2))
        rm = self._out((N,))
        its, acc, st = (self._out((N,), torch.int32) for _ in range(3))
        ws = self._out((min(chunk, N) * per_row,), torch.uint8)
        wv = (C.c_float * 3)(*w)
        for r0, n, at in row_chunks(N, chunk):
            self._call("avae_motion_track", at(p), at(q0), n, T, D, frames.data_ptr(), axes.data_ptr(), dt, wv, R, ptr(E), ptr(lim),
                       wl, n_iters, lam0, TRACK_FACTOR, TRACK_LAM_MIN, TRACK_LAM_MAX, tol, ws.data_ptr(), n * per_row, at(traj),
                       at(ctrl) if T > 1 else None, at(c0), at(c1), at(rm), at(its), at(acc), at(st))
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
        example ``chain.mass_matrix(seed)``, the arm's inertia at the seed pose: ``effort_weight |M(seed) u|^2`` is the reference's
        effort term with its ``M(q_t)`` frozen at one pose (``motion_effort`` prices a result with the moving one).  ``limits``
        (True: the chain's own, None or ``[n_dof, 2]``) enter as a quadratic penalty ``limit_weight`` on what an angle lies outside them,
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
        path = self._out((N, T, 2))
        vel = self._out((N, T, 2)) if velocity else None
        for r0, n, at in row_chunks(N, self._lognormal_chunk):
            self._call("avae_lognormal_eval", at(p), at(cnt), at(st), n, Cn, T, dt, at(path), at(vel))
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
        out = self._out((N, Cn, 6))
        l0, l1 = (self._out((N,), torch.float64) for _ in range(2))
        its, acc, stt = (self._out((N,), torch.int32) for _ in range(3))
        per_row = fr is not None and fr.dim() == 3
        for r0, n, at in row_chunks(N, self._lognormal_chunk):
            self._call("avae_lognormal_fit", at(s), at(p), at(cnt), at(st), n, Cn, T, dt, n_iters, wp, wv, tol,
                       at(fr) if per_row else ptr(fr), 1 if per_row else 0, ptr(lo), ptr(hi), at(out), at(l0), at(l1), at(its),
                       at(acc), at(stt))
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
        out = self._out((N, S, T, 2))
        pert = self._out((N, S, Cn, 6)) if want_params else None
        for r0, n, at in row_chunks(N, int(self._lognormal_chunk) // S):
            self._call("avae_lognormal_sample", at(p), at(cnt), at(st), n, S, Cn, T, dt, seed, r0, amplitude, angle, straightness,
                       1 if shift_mean else 0, at(out), at(pert))
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


# ---------------------------------------------------------------------- gradients of the writing chain
# Functions of a model, not methods: the class's surface is pinned name by name (tests/test_surface_cpu.py), and these reach the
# model through the same few members the mixin's methods use (``_call``, ``_out``, ``_like_input``, ``_motion_eval``, ``_motion_fk``,
# ``_render``, ``_encode``, ``_decode``).  ``vae_assoc_amd.vae_assoc`` and the package export the six public ones.
def _render_vjp(model, p, plane, canvas, target, height, g_image, g_img_l2, g_height_l2, objective=None):
    """avae_stroke_render_vjp on device tensors -> dict of device tensors: ``grad_path`` and the forward outputs (``img_l2`` /
    ``height_l2`` None without their input); ``objective [N]`` is filled in place where given"""
    N, T, H = p.shape[0], p.shape[1], canvas.size
    grad = model._out((N, T, 3))
    image, window = model._out((N, H * H)), model._out((N, 3))
    l2 = None if target is None else model._out(N)
    hl2 = None if height is None else model._out(N)
    if N:
        model._call("avae_stroke_render_vjp", p.data_ptr(), N, T, plane.data_ptr(), canvas.half_width, canvas.margin, H,
                    canvas.supersample, ptr(target), ptr(height), ptr(g_image), ptr(g_img_l2), ptr(g_height_l2), grad.data_ptr(),
                    image.data_ptr(), window.data_ptr(), ptr(l2), ptr(hl2), ptr(objective))
    return {"grad_path": grad, "image": image, "window": window, "img_l2": l2, "height_l2": hl2}


def _motion_fk_vjp(model, t, frames, axes, g):
    """avae_motion_fk_vjp on device tensors: trajectories [N, T, D] and the path's cotangent [N, T, 3] -> [N, T, D]"""
    N, T, D = t.shape
    out = model._out((N, T, D))
    if N:
        model._call("avae_motion_fk_vjp", t.data_ptr(), N, T, D, frames.data_ptr(), axes.data_ptr(), g.data_ptr(), out.data_ptr())
    return out


def _motion_eval_vjp(model, p, mats, basis, g):
    """avae_motion_eval_vjp on device tensors: parameters [N, P] and the trajectory's cotangent [N, T, D] -> [N, P]"""
    N = p.shape[0]
    out = model._out((N, basis.n_params))
    if N:
        model._call("avae_motion_eval_vjp", p.data_ptr(), N, basis.n_dof, basis.n_kb, basis.n_points, mats["phi"].data_ptr(),
                    ptr(mats["scale"]), ptr(mats["shift"]), ptr(mats["limits"]), ptr(mats["gain"]), ptr(mats["target"]), mats["nc"],
                    g.data_ptr(), out.data_ptr())
    return out


def _rows_adam(model, x, g, st, status, opts, cost=None):
    """avae_rows_adam in place on ``x [P, n]`` and the state ``st`` (``rows_adam_args``'); ``cost [P]`` feeds the best-so-far"""
    P, n = x.shape
    lr, b1, b2, eps, mn = opts
    if P:
        model._call("avae_rows_adam", x.data_ptr(), g.data_ptr(), st["m"].data_ptr(), st["v"].data_ptr(), st["t"].data_ptr(),
                    status.data_ptr(), P, n, lr, b1, b2, eps, mn, ptr(cost), ptr(None if cost is None else st["best_cost"]),
                    ptr(None if cost is None else st["best_x"]))


def render_strokes_vjp(model, path, canvas, g_image=None, g_img_l2=None, g_height_l2=None, target=None, height=None):
    """The vector-Jacobian product of ``render_strokes`` (avae_stroke_render_vjp in include/avae.h): the gradient of
    ``sum g_image . image + g_img_l2 img_l2 + g_height_l2 height_l2`` with respect to ``path [N, T, 3]``.  ``g_image`` is
    ``[N, size * size]``, ``g_img_l2`` and ``g_height_l2`` ``[N]`` or one number; each may be None, and a distance's cotangent
    needs ``target`` / ``height`` as ``render_strokes`` takes them.  The renderer is piecewise smooth: the gradient is the one
    of the piece the path lies in (which segment is nearest to a sample, which points are the outermost, which samples lie on
    the edge ramp).  Returns ``render_strokes``' dict with ``grad_path [N, T, 3]`` added; the forward outputs are bitwise
    ``render_strokes``'.  A row's gradient is the same bits alone or among other rows and on repetition."""
    p, plane, tg, hg, gi, gl, gh, was_np = render_vjp_args(path, canvas, target, height, g_image, g_img_l2, g_height_l2,
                                                           model.device)
    conv = model._like_input(was_np)
    return {k: conv(v) for k, v in _render_vjp(model, p, plane, canvas, tg, hg, gi, gl, gh).items()}


def motion_fk_vjp(model, trajectories, chain, grad_path):
    """The vector-Jacobian product of ``motion_fk`` (avae_motion_fk_vjp): the pen path's cotangent ``grad_path [N, T, 3]`` ->
    the joint angles' ``[N, T, chain.n_dof]``, ``(axis_j x (tip - origin_j)) . grad_path`` per joint -- the position rows of
    ``motion_pose``'s Jacobian, contracted without ever forming them."""
    t, frames, axes, g, was_np = motion_fk_vjp_args(trajectories, chain, grad_path, model.device)
    return model._like_input(was_np)(_motion_fk_vjp(model, t, frames, axes, g))


def motion_eval_vjp(model, params, basis, grad_trajectory, anchor=None):
    """The vector-Jacobian product of ``motion_eval`` (avae_motion_eval_vjp): the trajectory's cotangent ``grad_trajectory
    [N, n_points, n_dof]`` -> the standardised parameters' ``[N, basis.n_params]``.  A point the joint limits clamped passes
    nothing on; ``anchor`` as in ``motion_eval`` (its target is a constant of the parameters)."""
    p, mats, g, was_np = motion_eval_vjp_args(params, basis, anchor, grad_trajectory, model.device)
    return model._like_input(was_np)(_motion_eval_vjp(model, p, mats, basis, g))


def rows_adam(model, x, grad, state=None, lr=0.05, betas=(0.9, 0.999), eps=1e-8, max_norm=None, cost=None):
    """One Adam step for P independent problems at once (avae_rows_adam): ``x`` and ``grad`` are ``[P, n]``, n <= 1024.  A row
    whose gradient holds a NaN or Inf is left as it is (status 2); otherwise the gradient is scaled by ``min(1, max_norm /
    |grad|)`` (``max_norm`` None: not at all) and the bias-corrected update uses the row's own step count.  ``cost [P]`` is the
    cost at ``x``: where it is below the state's ``best_cost``, ``x`` is kept as ``best_x`` first.  Returns a dict of ``x`` (the
    new point; the input is not changed), ``status [P]`` (int32) and ``state`` (``m``, ``v``, ``t``, ``best_x``, ``best_cost`` on
    the device) to pass to the next step."""
    opts = adam_options(lr, betas, eps, max_norm)
    xt, g, st, c, was_np = rows_adam_args(x, grad, state, cost, model.device)
    status = torch.zeros(xt.shape[0], dtype=torch.int32, device=model.device)
    _rows_adam(model, xt, g, st, status, opts, c)
    conv = model._like_input(was_np)
    return {"x": conv(xt), "status": conv(status), "state": st}


def _cost_cotangents(model, w, N):
    """the cotangents of ``img_l2`` and ``height_l2`` under ``cost = w0 (img_l2 + w1 height_l2)``, [N] each"""
    return (torch.full((N,), w[0], dtype=torch.float32, device=model.device),
            torch.full((N,), w[0] * w[1], dtype=torch.float32, device=model.device))


def writing_cost_grad(model, params, basis, chain, canvas, target_image, height=None, weights=(0.3, 10.0), anchor=None):
    """The differentiable part of ``writing_cost`` and its gradient: ``cost = w0 (img_l2 + w1 height_l2)`` of the drawing of
    each row of ``params`` against ``target_image``, and ``grad [N, n_params]``, its derivative with respect to the
    standardised parameters -- ``motion_eval``, ``motion_fk`` and the three reverse launches, at about the price of two
    drawings.  ``height=None`` is the row's own mean height, as in ``writing_cost`` (the mean's own derivative vanishes: the
    residuals sum to 0).  The latent term of ``writing_cost`` is not part of this cost: its gradient needs the encoder's
    derivative with respect to its input, which no launch of the library forms.  Returns a dict of ``cost``, ``img_l2``,
    ``height_l2 [N]``, ``grad`` and ``image``; the three forward pieces are bitwise ``draw_motion``'s."""
    w = cost_weights(weights)
    if target_image is None:
        raise ValueError("target_image is None: the cost needs the picture to compare with")
    p, mats, frames, axes, plane, tg, hg, was_np = draw_args(params, basis, chain, canvas, anchor, target_image, height,
                                                             model.device)
    traj = model._motion_eval(p, mats, basis)[0]
    path = model._motion_fk(traj, frames, axes)
    if hg is None:
        hg = (path @ plane[2]).mean(1).contiguous()
    gl, gh = _cost_cotangents(model, w, int(p.shape[0]))
    out = _render_vjp(model, path, plane, canvas, tg, hg, None, gl, gh)
    grad = _motion_eval_vjp(model, p, mats, basis, _motion_fk_vjp(model, traj, frames, axes, out["grad_path"]))
    cost = w[0] * (out["img_l2"] + w[1] * out["height_l2"])
    conv = model._like_input(was_np)
    return {"cost": conv(cost), "img_l2": conv(out["img_l2"]), "height_l2": conv(out["height_l2"]), "grad": conv(grad),
            "image": conv(out["image"])}


def descend_motion(model, target_image, basis, chain, canvas, init=None, n_iters=50, lr=0.05, max_norm=None, anchor_start=True,
                   weights=(0.3, 10.0), modality=1, state=None, image_modality=0):
    """Gradient refinement of a written motion for P pictures at once: Adam on ``writing_cost_grad``'s cost, the descent
    ``refine_motion(space='params')`` searches for.

    It starts where that search starts: the motion decoded from the encoding of ``target_image [P, n_pixels]`` (or ``init
    [P, n_params]``), priced at the mean pen height of that first motion; with ``anchor_start`` the parameters are read
    through the projection onto starting where the first trajectory starts (``motion_eval``'s ``anchor``).  An iteration is
    six launches -- ``motion_eval``, ``motion_fk``, the three reverse passes and ``rows_adam`` (``lr``, ``max_norm``) -- and
    nothing is read back to the host inside the loop.

    Returns a dict: ``params`` (after the last step) and ``best_params [P, n_params]`` (the cheapest point visited, the
    last included), ``cost``, ``img_l2``, ``height_l2`` and ``image`` at ``params``, ``best_cost [P]`` and ``best_image``,
    ``history [n_iters + 1, P]`` (the cost before every step and after the last), ``status [P]`` (int32, of the last step:
    0, or 2 where the gradient was not finite and the row stayed), ``height [P]`` and ``state``.
    ``descend_motion(..., state=state)`` continues the run (``init`` is then ignored): k iterations and then m more are the
    bits of k + m.  NumPy in gives NumPy out (``state`` stays on the device)."""
    n_iters, opts, w = descend_motion_args(basis, chain, canvas, n_iters, lr, max_norm, anchor_start, weights, modality,
                                           image_modality, model._widths)
    if target_image is None:
        raise ValueError("target_image is None: the refinement needs the pictures to write")
    tg, was_np = dev_array(target_image, canvas.n_pixels, model.device)
    tg = tg.contiguous()
    P = int(tg.shape[0])
    frames, axes = chain_matrices(chain, model.device)
    plane = canvas_args(canvas, P, None, None, model.device)[0]
    if state is None:
        p0 = dev_dense(init, basis.n_params, model.device, P, "as target_image", name="init")
        if p0 is None:
            p0 = model._decode(modality, model._encode(image_modality, tg))
        traj0 = model._motion_eval(p0, motion_matrices(basis, model.device), basis)[0]
        h0 = (model._motion_fk(traj0, frames, axes) @ plane[2]).mean(1).contiguous()
        st = dict(params=p0.clone().contiguous(), height=h0, iteration=0,
                  anchor=traj0[:, 0, :].reshape(P, basis.n_dof, 1).contiguous() if anchor_start else None,
                  adam=rows_adam_args(p0, p0, None, None, model.device)[2])
    else:
        st = descent_state(state, P, basis, model.device)
    anchor = None if st["anchor"] is None else dict(phases=[0.0], target=st["anchor"])
    mats = motion_matrices(basis, model.device, anchor, P)
    x, h0, adam = st["params"], st["height"], st["adam"]
    gl, gh = _cost_cotangents(model, w, P)
    hist = torch.full((n_iters + 1, P), float("nan"), dtype=torch.float32, device=model.device)
    status = torch.zeros(P, dtype=torch.int32, device=model.device)

    def reverse(i):
        traj = model._motion_eval(x, mats, basis)[0]
        out = _render_vjp(model, model._motion_fk(traj, frames, axes), plane, canvas, tg, h0, None, gl, gh, hist[i])
        return traj, out
    for i in range(n_iters if P else 0):
        traj, out = reverse(i)
        g = _motion_eval_vjp(model, x, mats, basis, _motion_fk_vjp(model, traj, frames, axes, out["grad_path"]))
        _rows_adam(model, x, g, adam, status, opts, hist[i])
    st["iteration"] += n_iters
    _, last = reverse(n_iters)
    better = hist[n_iters] < adam["best_cost"]
    best_x = torch.where(better[:, None], x, adam["best_x"])
    best_cost = torch.where(better, hist[n_iters], adam["best_cost"])
    best = model._render(model._motion_fk(model._motion_eval(best_x, mats, basis)[0], frames, axes), plane, canvas, None, None)
    conv = model._like_input(was_np)
    return {"params": conv(x.clone()), "best_params": conv(best_x), "cost": conv(hist[n_iters].clone()),
            "img_l2": conv(last["img_l2"]), "height_l2": conv(last["height_l2"]), "image": conv(last["image"]),
            "best_cost": conv(best_cost), "best_image": conv(best["image"]), "history": conv(hist), "status": conv(status),
            "height": conv(h0), "state": st}


# ---------------------------------------------------------------------------------------------------- rigid-body dynamics (section 32)
def _motion_dynamics(model, t, v, a, frames, axes, bodies, gravity, inertia=False, gravity_torque=True, coriolis=True, torque=True):
    """avae_motion_dynamics on device tensors: trajectories, speeds and accelerations [N, T, D] (the last two may be None) ->
    (inertia [N, T, D, D], gravity, coriolis, torque [N, T, D]), None for an output that is not asked for"""
    N, T, D = t.shape

    def new(want, *tail):
        return model._out((N, T, D) + tail) if want else None
    M, g, c, tau = new(inertia, D), new(gravity_torque), new(coriolis), new(torque)
    if N:
        model._call("avae_motion_dynamics", t.data_ptr(), ptr(v), ptr(a), N, T, D, frames.data_ptr(), axes.data_ptr(),
                    bodies.data_ptr(), (C.c_float * 3)(*gravity), ptr(M), ptr(g), ptr(c), ptr(tau))
    return M, g, c, tau


def _differences(t, dt):
    """``motion_track``'s finite differences of trajectories [N, T, D] on the device -> (v, a): ``v_0 = 0``, ``v_t = (q_t -
    q_(t-1)) / dt``, ``a_t = (v_(t+1) - v_t) / dt``, ``a_(T-1) = 0``, float32 differences and divisions (``dt`` as a device
    scalar: a host scalar would turn the division into a product with 1 / dt)"""
    v, a = torch.zeros_like(t), torch.zeros_like(t)
    dt = torch.full((), dt, dtype=t.dtype, device=t.device)
    v[:, 1:] = (t[:, 1:] - t[:, :-1]) / dt
    a[:, :-1] = (v[:, 1:] - v[:, :-1]) / dt
    return v, a


def motion_dynamics(model, trajectories, chain, velocities=None, accelerations=None, dt=None, gravity=(0.0, 0.0, -9.81),
                    inertia=False):
    """The joint torques a motion asks of the arm (avae_motion_dynamics in include/avae.h): the reference's ``baxter_dynamics``
    (``inertia``, ``coriolis``, ``gravity`` of baxter_pykdl_revised.py:218-296) for every point of N trajectories ``[N, T,
    chain.n_dof]`` in one launch.  ``chain`` must carry inertial data (``KinematicChain.has_inertia``).  ``velocities`` and
    ``accelerations`` (the trajectories' shape; None: zeros) are the joint speeds and accelerations at each point; with ``dt``
    given and neither of them they are ``motion_track``'s finite differences of the trajectory (``v_0 = 0``, ``v_t = (q_t -
    q_(t-1)) / dt``, ``a_t = (v_(t+1) - v_t) / dt``, ``a_(T-1) = 0``), formed on the device.  ``gravity`` is the acceleration
    of free fall in the base frame.

    Returns a dict: ``torque [N, T, n_dof]`` (``M a + c + g``), ``gravity`` (g alone) and ``coriolis`` (c alone: the torque at
    ``a = 0`` without gravity), with ``inertia=True`` also ``inertia [N, T, n_dof, n_dof]`` (M, symmetric bit for bit), and,
    when every joint of the chain has an effort limit, ``peak_torque [N, n_dof]`` (``max_t |torque|``) and ``torque_ratio
    [N, n_dof]`` (that over the limit: a motion stays within the arm's torques where it is at most 1).  A point with a
    non-finite angle, speed or acceleration is NaN in its own outputs.  NumPy in gives NumPy out, device tensors in give
    device tensors out."""
    t, v, a, dt, frames, axes, bodies, grav, lim, want, was_np = motion_dynamics_args(trajectories, chain, velocities, accelerations,
                                                                                      dt, gravity, inertia, model.device)
    if dt is not None:
        v, a = _differences(t, dt)
    M, g, c, tau = _motion_dynamics(model, t, v, a, frames, axes, bodies, grav, inertia=want)
    conv = model._like_input(was_np)
    out = {"torque": conv(tau), "gravity": conv(g), "coriolis": conv(c)}
    if want:
        out["inertia"] = conv(M)
    if lim is not None:
        peak = tau.abs().amax(1) if tau.shape[0] else tau.new_zeros((0, tau.shape[2]))
        out.update(peak_torque=conv(peak), torque_ratio=conv(peak / lim))
    return out


def motion_effort(model, trajectories, chain, dt=0.01):
    """The reference's control effort of N trajectories ``[N, T, chain.n_dof]``, whoever made them (``ctrl_effort``,
    baxter_writer.py:112-126): ``effort [N] = sum_(t < T - 1) |M(q_t) u_t|^2`` with ``M`` the joint-space inertia at the pose of
    time point t and ``u_t`` ``motion_track``'s controls of the trajectory, the finite differences ``motion_dynamics`` forms
    with ``dt``.  ``M(q_t) u_t`` is one ``avae_motion_dynamics`` launch (speeds left out, no gravity); squares and sums are
    torch reductions on the device.  Returns a dict of ``effort [N]`` and ``controls [N, T - 1, n_dof]``."""
    t, dt, frames, axes, bodies, was_np = motion_effort_args(trajectories, chain, dt, model.device)
    u = _differences(t, dt)[1]
    tau = _motion_dynamics(model, t, None, u, frames, axes, bodies, (0.0, 0.0, 0.0), gravity_torque=False, coriolis=False)[3]
    conv = model._like_input(was_np)
    return {"effort": conv((tau[:, :-1] * tau[:, :-1]).sum((1, 2))), "controls": conv(u[:, :-1].contiguous())}
