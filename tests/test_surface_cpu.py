"""The surface of ``AssocVariationalAutoEncoder`` and of the module ``vae_assoc_amd.vae_assoc``, pinned: every callable attribute
of the class with its signature, the class-level knobs with their values and every module-level name, as recorded with
``inspect`` on the commit before the class was spread over ``vae_assoc``, ``_latent_api`` and ``_pen_api``.  Moving a method
between those modules must leave this table alone.  Needs neither a GPU nor libavae.so."""
import inspect

import vae_assoc_amd.vae_assoc as V

# the differences from the recorded commit, by name: the shared call and allocation helpers came, ``_new`` (2-D float only) went
ADDED = {"_call": "(self, name, *args)", "_call_host": "(self, name, *args)", "_out": "(self, shape, dtype=torch.float32)"}
REMOVED = {"_new"}

SIGNATURES = {
    '_apply': '(self, want_cost=True)',
    '_apply_bucket': '(self, b, want_cost=True)',
    '_backward': '(self, X, eps=None, inputs=None)',
    '_backward_bucket': '(self, b)',
    '_batch_args': '(self, X, eps, n_steps=1, present=None, inputs=None)',
    '_call_in': '(self, name, head, ins, p, tail)',
    '_decode': '(self, modality, z, out=None)',
    '_encode': '(self, m, x, want_logvar=False)',
    '_fused_decode': '(self, xp, lds, p, rows, modality, want_mean)',
    '_gmm_fit': '(self, mu, lv, K, n_iters, var_floor, w, m, s)',
    '_grad_tensor': '(self)',
    '_letter_thumbnails': '(self, t, row, frame, flags, thr, size)',
    '_like_input': '(was_np)',
    '_loglik': '(self, X, present, n_samples, eps)',
    '_lognormal_eval': '(self, p, cnt, st, T, dt, velocity=True)',
    '_lognormal_fit': '(self, s, p, cnt, st, dt, opts, fr, lo, hi)',
    '_lognormal_sample': '(self, p, cnt, st, T, dt, S, seed, amplitude, angle, straightness, shift_mean, want_params=True)',
    '_motion_eval': '(self, p, mats, basis, ref=None, refp=None)',
    '_motion_fit': '(self, t, pinv, sc, sh, basis)',
    '_motion_fk': '(self, t, frames, axes)',
    '_motion_ik': '(self, p, frames, axes, seed, orient, lim, opts)',
    '_motion_moments': '(self, s, N, S, mats, basis, mean, var, frac)',
    '_motion_pose': '(self, t, frames, axes, position=True, rotation=True, jacobian=False)',
    '_motion_track': '(self, p, frames, axes, q0, E, lim, opts)',
    '_new': '(self, rows, cols)',
    '_ptrs': '(ts)',
    '_render': '(self, p, plane, canvas, target, height)',
    '_score': '(self, X, present, eps, cross_modal)',
    '_search_sample': '(self, st, R, seed, iteration, proj, x)',
    '_search_update': '(self, st, x, c, opt, avg=None, mn=None, moved=None)',
    '_smoothed': '(self, p, chain, traj, tr)',
    '_stage': '(self, X, eps=None, n_steps=1, inputs=None)',
    '_stage_run': '(self, n, ts, lds, e, ins, i0)',
    '_stream': '(self)',
    '_train': '(self, X, n_steps, eps, present, return_cost, one_step=False, inputs=None)',
    '_twin': '(self, name, head, p, tail)',
    '_writing_cost': '(self, p, mats, basis, frames, axes, plane, canvas, tg, hg, zt, w, image_modality)',
    'aggregate_log_density': '(self, z, gallery, exclude=None, marginals=True)',
    'averaged': '(self)',
    'complete': '(self, X, observed=None, n_iters=50, lr=0.05, prior_weight=1.0, z0=None, init=None)',
    'cost_history': '(self, n)',
    'cycle_error': '(self, X, basis, chain, canvas, source=0, modality=1)',
    'draw_motion': '(self, params, basis, chain, canvas, anchor=None, target=None, height=None)',
    'elbo_decomposition': '(self, X, n_samples=1, eps=None, seed=0, leave_one_out=False)',
    'embed_latents': "(self, posteriors, perplexity=30.0, n_iters=1000, metric='symkl', learning_rate='auto', early_exaggeration=12.0, "
                     'exaggeration_iters=250, momentum=(0.5, 0.8), init=None, seed=0, state=None)',
    'evaluate_cost': '(self, X, eps=None, present=None, inputs=None)',
    'fit_latent_prior': '(self, posteriors, n_components=10, n_iters=50, init=None, seed=0, var_floor=1e-06)',
    'frames_to_motion': '(self, frames, basis, image_modality=0, modality=1, **thumbnail_options)',
    'generate': '(self, z_mu=None)',
    'get_ema_params': '(self)',
    'get_grads': '(self)',
    'get_opt_state': '(self)',
    'get_params': '(self)',
    'grad_norm_history': '(self, n)',
    'hyper_history': '(self, n)',
    'impute': '(self, X, present=None, n_samples=0, eps=None)',
    'latent_diagnostics': '(self, X, present=None, au_threshold=0.01)',
    'latent_map': '(self, X, **kw)',
    'latent_prior_score': '(self, z, prior, responsibilities=False)',
    'latent_stats': '(self, posteriors, present=None)',
    'latent_topk': "(self, query, gallery, k=1, metric='symkl')",
    'letter_thumbnails': "(self, frames, size=28, threshold=None, invert=False, channel_order='rgb')",
    'log_likelihood': '(self, X, n_samples=64, eps=None)',
    'log_likelihood_masked': '(self, X, present, n_samples=64, eps=None)',
    'lognormal_augment': '(self, strokes=None, params=None, count=None, n_samples=10, seed=0, amplitude=0.2, angle=0.3490658503988659, '
                         'straightness=0.1, shift_mean=True, start=None, dt=None, n_points=None, **fit_options)',
    'lognormal_eval': '(self, params, n_points, count=None, start=None, dt=None)',
    'lognormal_fit': '(self, strokes, init=None, count=None, start=None, dt=None, max_components=8, n_iters=40, weights=(1.0, 0.001), '
                     'free=None, bounds=None, tol=1e-09)',
    'motion_error': '(self, X, basis, source=0, modality=1)',
    'motion_eval': '(self, params, basis, anchor=None, reference=None, reference_params=None)',
    'motion_fit': '(self, trajectories, basis)',
    'motion_fk': '(self, trajectories, chain)',
    'motion_ik': '(self, path, chain, seed, orientation=None, n_iters=20, tol=1e-05, rot_tol=0.0001, damping=0.01, max_step=0.5, '
                 'limits=True)',
    'motion_moments': '(self, samples, basis, anchor=None)',
    'motion_pose': '(self, trajectories, chain, jacobian=False)',
    'motion_track': '(self, path, chain, seed=None, init=None, orientation=None, dt=0.01, track_weights=(10.0, 10.0, 50.0), '
                    'effort_weight=0.01, effort=None, limits=True, limit_weight=0.0, n_iters=25, lam0=1.0, tol=1e-06, ik_options=None)',
    'partial_fit': '(self, X, eps=None, return_cost=True, present=None, inputs=None)',
    'partial_fit_steps': '(self, X, n_steps, eps=None, return_cost=True, present=None, inputs=None)',
    'posterior': '(self, X, sens_idx=None)',
    'predict_motion': '(self, X, basis, modality=1, present=None, n_samples=0, eps=None, anchor=None)',
    'reconstruct': '(self, X, eps=None)',
    'refine_motion': "(self, target_image, basis, chain, canvas, space='latent', init=None, n_rollouts=None, n_iters=10, var0=None, "
                     'anchor_start=True, weights=(0.3, 10.0, 0.7), image_modality=0, modality=1, **search_options)',
    'refine_pen_path': '(self, target_image, basis, chain, canvas, init=None, n_rollouts=50, n_iters=20, var0=1e-05, anchor_start=True, '
                       "seed_angles=None, image_modality=0, modality=1, ik_n_iters=20, solver='ik', track_options=None, **options)",
    'render_strokes': '(self, path, canvas, target=None, height=None)',
    'restore_model': '(self, folder=None, fname=None)',
    'retrieval_recall': "(self, X, ks=(1, 5, 10), metric='symkl')",
    'retrieve': "(self, X, sens_idx, gallery, k=1, metric='symkl')",
    'sample_latent_prior': '(self, prior, n, seed=0)',
    'save_model': '(self, fname=None)',
    'score_samples': '(self, X, eps=None, cross_modal=False)',
    'score_samples_masked': '(self, X, present, eps=None, cross_modal=False)',
    'search': "(self, cost, x0, var0, n_rollouts=10, n_iters=10, eliteness=10, weighting='PI-BB', cov_update='PI-BB', learning_rate=1.0, "
              'covar_bounds=(0.1,), tol=1e-06, project=None, seed=0, state=None)',
    'set_corruption': '(self, drop=0.0, noise=0.0, drop_value=0.0)',
    'set_ema': '(self, decay, warmup=False)',
    'set_ema_params': '(self, flat)',
    'set_grad_clip': '(self, max_norm=0.0, skip_nonfinite=False)',
    'set_opt_state': '(self, m=None, v=None, step=0)',
    'set_params': '(self, flat)',
    'set_schedule': '(self, kl=None, assoc=None, lr=None)',
    'strokes_to_motion': "(self, strokes, basis, chain, canvas, center, seed, height=0.0, solver='ik', track_options=None, **ik_options)",
    'synchronize': '(self)',
    'transform': '(self, X, sens_idx=None)',
    'use_averaged': '(self, on=True)',
    'writing_cost': '(self, params, basis, chain, canvas, target_image, target_latent=None, height=None, weights=(0.3, 10.0, 0.7), '
                    'image_modality=0)',
}

DATA = {
    'STATS_SHAPES': (('count', 'MM'), ('mean', 'MMz'), ('var', 'MMz'), ('xcov', 'MMz'), ('assoc', 'MMz'), ('post_var', 'Mz'),
                     ('kl', 'Mz'), ('cov', 'Mzz')),
    '_lognormal_chunk': 16384,
    '_motion_chunk': 16384,
    '_track_chunk': None,
}

MODULE_NAMES = [
    'AssocVariationalAutoEncoder', 'C', 'GradSync', 'MotionBasis', 'SEARCH_STATE_KEYS', 'THUMBNAIL_CAMERA', 'THUMBNAIL_CANVAS',
    'TRACK_FACTOR', 'TRACK_LAM_MAX', 'TRACK_LAM_MIN', '_ARCH_KEYS', '_act_name', '_capi', '_is_pair', '_same_joints', 'agg_args',
    'as_index', 'build_config', 'canvas_args', 'chain_matrices', 'check_solver', 'contextlib', 'corruption_fields', 'create_replica',
    'cyclical', 'datetime', 'dev_array', 'dev_block3', 'dev_dense', 'dev_dense3', 'dev_flags', 'dev_inputs', 'dev_modalities',
    'dev_row_args', 'dp_bucket_schedule', 'dp_train_step_bucketed', 'draw_args', 'ema_fields', 'ema_kwargs', 'embed_args',
    'exponential_decay', 'grad_clip_fields', 'grad_clip_kwargs', 'hidden_sizes', 'impute_args', 'initial_params', 'latent_prior_args',
    'latent_score_args', 'latent_stats_args', 'layer_shapes', 'ld_of', 'letter_thumbnail_args', 'linear_warmup',
    'lognormal_augment_args', 'lognormal_eval_args', 'lognormal_fit_args', 'lognormal_sample_options', 'motion_eval_args',
    'motion_fit_args', 'motion_fk_args', 'motion_ik_args', 'motion_matrices', 'motion_moments_args', 'motion_pose_args',
    'motion_track_args', 'np', 'occlude_quadrant', 'os', 'predict_motion_args', 'prior_arrays', 'ptr', 'refine_motion_args',
    'refine_pen_path_args', 'render_args', 'schedule_kwargs', 'schedule_struct', 'search_args', 'strokes_to_motion_args', 'time',
    'to_device32', 'topk_args', 'torch', 'track_rows_per_call', 'train', 'train_loop', 'writing_cost_args', 'xavier_init',
]


def _surface(cls):
    """-> (callable attributes with their signatures, the other attributes with their values), dunder names left out"""
    sigs, data = {}, {}
    for name in dir(cls):
        if name.startswith("__") and name.endswith("__"):
            continue
        v = getattr(cls, name)
        if callable(v):
            sigs[name] = str(inspect.signature(v))
        else:
            data[name] = v
    return sigs, data


def test_the_class_has_exactly_the_recorded_callables_and_knobs():
    sigs, data = _surface(V.AssocVariationalAutoEncoder)
    assert len(SIGNATURES) == 103 and REMOVED <= set(SIGNATURES) and not set(ADDED) & set(SIGNATURES)
    want = {k: s for k, s in SIGNATURES.items() if k not in REMOVED}
    want.update(ADDED)
    assert set(sigs) == set(want), (sorted(set(sigs) - set(want)), sorted(set(want) - set(sigs)))
    wrong = {k: (sigs[k], want[k]) for k in want if sigs[k] != want[k]}
    assert not wrong, wrong
    assert data == DATA
    cls = V.AssocVariationalAutoEncoder
    assert cls.letter_thumbnails.CAMERA == {"threshold": 108, "invert": True} and cls.letter_thumbnails.CANVAS == {"invert": True}


def test_every_recorded_module_name_is_still_importable():
    missing = [n for n in MODULE_NAMES if not hasattr(V, n)]
    assert len(MODULE_NAMES) == 87 and not missing, missing
