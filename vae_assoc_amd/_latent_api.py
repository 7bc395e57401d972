"""The latent-analysis methods of ``AssocVariationalAutoEncoder`` (DESIGN.md sections 18-22): cross-modal retrieval, posterior
diagnostics, the aggregate posterior, the mixture prior and the t-SNE map of the codes.

``LatentAPI`` is a mixin of ``vae_assoc.AssocVariationalAutoEncoder``: its methods reach the model through ``self`` alone
(``_encode``, ``_call``, ``_out``, ``_ptrs``, ``_like_input``), and this module imports nothing from ``vae_assoc``."""
import ctypes as C

import numpy as np
import torch

from . import _capi
from ._args import agg_args, embed_args, latent_prior_args, latent_score_args, latent_stats_args, prior_arrays, topk_args
from ._marshal import dev_array, dev_dense3, dev_flags, dev_modalities, ptr


class LatentAPI(object):
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
        index = self._out((rows, k), torch.int32)
        dist = self._out((rows, k))
        if rows:
            self._call("avae_latent_topk", qm.data_ptr(), ptr(ql), rows, gm.data_ptr(), ptr(gl), gm.shape[0], mid, k,
                       index.data_ptr(), dist.data_ptr())
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
        res = {name: self._out([dims[c] for c in shape], torch.int64 if name == "count" else torch.float64)
               for name, shape in self.STATS_SHAPES}
        out = _capi.LatentStatsOut(**{name: t.data_ptr() for name, t in res.items()})
        self._call("avae_latent_stats", len(mus), self._ptrs(mus), self._ptrs(lvs), ptr(p), rows, C.byref(out))
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
        joint = self._out((rows,))
        marginal = self._out((rows, self.n_z)) if marg else None
        if rows:
            self._call("avae_agg_logpdf", zt.data_ptr(), rows, ptr(gm), ptr(gl), gm.shape[0], ptr(ex), joint.data_ptr(),
                       ptr(marginal))
        conv = self._like_input(was_np)
        return {"joint": conv(joint), "marginal": conv(marginal)}

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
        bound = self._out((n_iters + 1,), torch.float64)
        n_used = self._out((1,), torch.int32)
        self._call("avae_gmm_fit", ptr(mu), ptr(lv), mu.shape[0], K, n_iters, var_floor, w.data_ptr(), m.data_ptr(), s.data_ptr(),
                   bound.data_ptr(), n_used.data_ptr())
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
        ll = self._out((rows,))
        comp = self._out((rows,), torch.int32)
        resp = self._out((rows, K)) if responsibilities else None
        if rows:
            self._call("avae_gmm_score", mu.data_ptr(), ptr(lv), rows, K, w.data_ptr(), m.data_ptr(), s.data_ptr(), ll.data_ptr(),
                       comp.data_ptr(), ptr(resp))
        conv = self._like_input(was_np)
        return {"log_density": conv(ll), "component": conv(comp), "responsibilities": conv(resp)}

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
            comp = self._out((0,), torch.int64)
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
            beta, shift, norm = (self._out((N,)) for _ in range(3))
            tries, n_used = self._out((N,), torch.int32), self._out((1,), torch.int32)
            self._call("avae_embed_calibrate", mu.data_ptr(), ptr(lv), N, a["metric"], a["perplexity"], 1e-5, 64, beta.data_ptr(),
                       shift.data_ptr(), norm.data_ptr(), tries.data_ptr(), n_used.data_ptr())
        else:
            beta, shift, norm = a["calibration"]
        y, vel, gain, T = a["y"], a["vel"], a["gain"], a["n_iters"]
        kl = self._out((T + 1,), torch.float64)
        self._call("avae_embed_iterate", mu.data_ptr(), ptr(lv), N, a["metric"], beta.data_ptr(), shift.data_ptr(), norm.data_ptr(),
                   y.data_ptr(), vel.data_ptr(), gain.data_ptr(), a["it0"], T, a["learning_rate"], a["early_exaggeration"],
                   a["exaggeration_iters"], a["momentum"][0], a["momentum"][1], 1, kl.data_ptr(), None)
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
