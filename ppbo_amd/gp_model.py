"""Drop-in GPModel: the reference's object surface (src/gp_model.py) on top of libppbo_hip.so.

Same constructor, methods, argument meaning and print-and-continue error behaviour as the
reference class; every O(N^2)/O(N^3)/O(M N^2) operation is a HIP kernel behind the C-ABI:
  update_Sigma       -> ppbo_gram            (gp_model.py:157-158, kernels.py, misc.py:71-88)
  update_Sigma_inv   -> ppbo_pd_inverse      (gp_model.py:161-162, misc.py:96-100)
  update_fMAP        -> ppbo_fit_fmap        (gp_model.py:354-389)
  Lambda / posterior -> ppbo_posterior       (gp_model.py:111-117, 249-274)
  mu_pred / mu_Sigma_pred -> ppbo_predict / ppbo_predict_cov   (gp_model.py:441-461)
  mu_star            -> batched candidate search with on-device argmax (replaces the sequential
                        differential evolution of gp_model.py:415-437), then a bounded polish.
Large matrices live on the GPU; the NumPy attributes other code reads (Sigma, Sigma_inv,
Lambda_MAP, posterior_covariance, ...) are materialised lazily on first access.
There is no CPU fallback: without the HIP library / a GPU the constructor raises.
"""
from __future__ import annotations

import time

import numpy as np
import scipy.optimize
import torch

from . import kernels as _kernels
from .engine import (ARD_KERNELS, CAMPHOR_ARD, NotPositiveDefinite, PAIR_MEAN, SCORE_MEAN, SCORE_POINTWISE_EI, SCORE_VARIANCE,
                     get_engine, lengthscales, theta_key)
from .feedback_processing import FeedbackProcessing

SEARCH_CANDIDATES = 65536      # uniform candidates per mu_star trial
ASCENT_STARTS = 32             # best well-separated candidates refined together on the device
ASCENT_ITERS = 100             # cap on ascent iterations per start (all inside one mean_ascent_kernel launch)
POLISH_GRAD_TOL = 1e-6         # |projected grad mu| / |mu| above which mu_star's winner gets the L-BFGS-B polish
PROFILE_CANDIDATES = 4096      # pool rows per box of a profile (profile_effect, profile_interaction): T boxes share one call
PROFILE_STARTS = 8             # ascents per box of a profile
ARD_FIT_GTOL = 1e-6            # optimize_theta_ard: f_MAP tolerance of each evaluation (the gradient's implicit term
                               # assumes grad T = 0; its error is of the order of |grad T|)
THETA_BOX = ((0.01, 2.0), (0.1, 15.0))    # the reference's search box for l and sigma_f (gp_model.py:397-398), sigma = 1
APPEND_REFRESH = 64            # incremental mode: bordered updates of Sigma^-1 between two full inversions (measured:
                               # 32 appends leave |Sigma Sigma^-1 - I| where a full inversion leaves it, 8.2e-8 at N = 2048)


def log_prior(theta):
    """The reference's log-prior of theta (gp_model.py:287-290): lognormal on sigma (s = 1, scale e), on the length scale
    (s = 0.5, scale e^-1.4) and on sigma_f (s = 0.5, scale e^1.7).  With per-dimension length scales the length-scale
    prior applies to each l_d and the terms are summed (independent priors); a scalar l gives the reference's value."""
    import scipy.stats
    l = theta[1]
    if np.ndim(l) == 0:
        lp_l = np.log(scipy.stats.lognorm.pdf(l, s=0.5, scale=np.exp(-1.4)))
    else:
        lp_l = float(np.sum(np.log(scipy.stats.lognorm.pdf(np.asarray(l, dtype=float), s=0.5, scale=np.exp(-1.4)))))
    return (np.log(scipy.stats.lognorm.pdf(theta[0], s=1, scale=np.exp(1))) + lp_l
            + np.log(scipy.stats.lognorm.pdf(theta[2], s=0.5, scale=np.exp(1.7))))


def log_prior_grad(theta):
    """Gradient of log_prior with respect to (l, sigma_f): each lognormal term gives -(1 + (ln x - ln scale) / s^2) / x.
    A scalar l gives two entries, a vector of D length scales D + 1."""
    l = np.ravel(np.asarray(theta[1], dtype=float))
    gl = -(1.0 + (np.log(l) + 1.4) / 0.25) / l
    sf = float(theta[2])
    return np.append(gl, -(1.0 + (np.log(sf) - 1.7) / 0.25) / sf)


def camphor_coordinate_sums(sums):
    """The evidence gradient's 11 per-column sums of camphor_copper_ard_kernel's embedded rows (c0, s0, c1, s1, z, c3, s3,
    c4, s4, c5, s5; include/ppbo_hip.h) -> one per coordinate: every column scales with 1 / l_d of its coordinate, so the
    cos and sin columns of a periodic coordinate add up."""
    s = np.asarray(sums, dtype=float)
    if s.shape != (11,):
        raise ValueError(f"camphor_coordinate_sums: 11 embedded-column sums, not {s.shape}")
    return np.array([s[0] + s[1], s[2] + s[3], s[4], s[5] + s[6], s[7] + s[8], s[9] + s[10]])


def _theta_list(theta):
    """[sigma, l, sigma_f] with floats, l a float or a float64 vector (per-dimension length scales)."""
    l = theta[1]
    return [float(theta[0]), float(l) if np.ndim(l) == 0 else np.asarray(l, dtype=float).copy(), float(theta[2])]


class GPModel:
    def __init__(self, PPBO_settings, engine=None, incremental=False, fMAP_method=None):
        """incremental=True (not a reference feature): when update_data() has only appended one
        query's m+1 rows (feedback_processing.py:133-154), Sigma^-1 is bordered instead of refactorised
        (ppbo_pd_inverse_append) and f_MAP starts from the previous estimate padded with the previous posterior
        mean at the new rows (the reference pads with the mean of f_MAP, gp_model.py:375-377, and only does so
        during initialisation; its default is a fresh prior draw per update)."""
        self.COVARIANCE_SHRINKAGE = 1e-6            # gp_model.py:26
        self.eng = engine if engine is not None else get_engine()
        self.incremental = bool(incremental)
        self._sinv_state = None      # (X copy, theta tuple, appends since the last full inversion) behind _dSigma_inv
        self.n_appends = 0           # bordered updates of Sigma^-1 actually performed (ppbo_pd_inverse_append)
        self.n_full_inversions = 0   # full potrf + trtri + GEMM inversions
        self.fMAP_restart_on_stall = False   # opt-in: refit from a fresh prior draw when the trust region stalls
        # mu_star ranks its 65536 candidates per trial by a posterior mean whose kernel values are evaluated in fp32
        # (ppbo_mean_search_multi, screen_fp32): the ranking only picks the ascents' starts, every reported value comes
        # from the fp64 ascent.  False: ranked by the fp64 mean (0.3 ms more per trial at C3).
        self.mustar_screen_fp32 = True
        self.polish_log = {"device_reascents": 0, "scipy_polishes": 0}    # how often mu_star's winners needed more than the ascent
        # "whitened": L-BFGS in z = L^-1 f finished by the trust region (ppbo_fit_fmap_whitened; O(N^2) per iteration; the
        # reference's optimum wherever T has one -- at sigma << sigma_f T has several local maxima and every local method,
        # SciPy's included, picks its own: DESIGN 5); anything else: the exact Newton trust region on f alone, which
        # follows SciPy trust-exact's iteration rules
        self.fMAP_method = fMAP_method if fMAP_method is not None else getattr(PPBO_settings, "fMAP_method", "whitened")
        # update_model(optimize_theta=True): "search" (optimize_theta) or "ard-gradient" (optimize_theta_ard)
        self.theta_optimizer = getattr(PPBO_settings, "theta_optimizer", "search")
        if self.fMAP_method not in ("whitened", "trust-region"):
            raise ValueError("fMAP_method must be 'whitened' or 'trust-region'")
        self.fit_log = []            # one dict per update_fMAP trial: iterations, n_cholesky, warm, seconds
        s = PPBO_settings
        self.verbose = s.verbose
        self.FP = None
        self.D = s.D
        self.original_bounds = s.original_bounds
        self.bounds = ((0, 1),) * self.D
        self.X = None
        self.N = None
        self.m = s.n_pseudoobservations
        self.obs_indices = self.pseudobs_indices = self.latest_obs_indices = None
        self.alpha_grid_distribution = s.alpha_grid_distribution
        self.TGN_speed = s.TGN_speed
        self.n_gausshermite_sample_points = s.n_gausshermite_sample_points
        self.xi_acquisition_function = s.xi_acquisition_function
        self.kernel = _kernels.BY_NAME[s.kernel]    # the reference eval()s the string (gp_model.py:48)
        self.theta_initial = s.theta_initial
        if self.theta_initial is not None and self.theta_initial[1] is not None:
            lengthscales(self.theta_initial, self.D, s.kernel)      # raises on a vector l the kernel / D cannot take
        self.theta = None
        self.fMAP = None
        self.fMAP_finding_trials = 1
        self.fMAP_optimizer = s.fMAP_optimizer
        self.fMAP_random_initial_vector = True
        self.fMAP_gtol = 1e-4                       # SciPy trust-exact default, which the reference inherits (gp_model.py:382-384)
        self.mustar_finding_trials = s.mustar_finding_trials
        self.mustar_previous_iteration = 0
        self.mustar = None
        self.xstar = None
        self.xstars_local = None
        self.initialization_running = True
        self.last_iteration = False
        self.skip_computations_during_initialization = s.skip_computations_during_initialization
        self.skip_xstaroptimization_during_initialization = s.skip_xstaroptimization_during_initialization
        self.fit_stats = None
        # device state
        self._dX = self._dSigma = self._dSigma_inv = self._dLinv = self._dL = None
        self._post = None           # engine.Posterior with G (variance operator)
        self._post_mean = None      # Posterior usable for the mean only (alpha current, no G)
        self._host = {}

    # ------------------------------------------------------------------ data
    def update_feedback_processing_object(self, X_obs):
        if self.FP is None:
            self.FP = FeedbackProcessing(self.D, self.m, self.original_bounds, self.alpha_grid_distribution,
                                         self.TGN_speed)
            self.FP.initialize_data(X_obs)
        else:
            self.FP.update_data(X_obs)

    def update_data(self):
        self.X = self.FP.X
        self.N = self.FP.N
        self.obs_indices = self.FP.obs_indices
        self.pseudobs_indices = self.FP.pseudobs_indices
        self.latest_obs_indices = self.FP.latest_obs_indices
        self._dX = self.eng.dev(self.X)

    def turn_initialization_off(self):
        self.initialization_running = False
        self.FP.alpha_grid_distribution = self.alpha_grid_distribution

    def set_last_iteration(self):
        self.last_iteration = True

    def is_pseudobs(self, i):
        return self.FP.is_pseudobs(i)

    # ------------------------------------------------------------------ lazily downloaded matrices
    def _lazy(self, key, make):
        if key not in self._host:
            self._host[key] = make()
        return self._host[key]

    def _invalidate(self, *keys):
        for k in keys:
            self._host.pop(k, None)

    @property
    def Sigma(self):
        return None if self._dSigma is None else self._lazy("Sigma", lambda: self._dSigma.cpu().numpy())

    @property
    def Sigma_inv(self):
        return None if self._dSigma_inv is None else self._lazy("Sigma_inv", lambda: self._dSigma_inv.cpu().numpy())

    @property
    def Lambda_MAP(self):
        if self._post is None:
            return None
        return self._lazy("Lambda_MAP", lambda: self._dense_lambda(self._post.lam_diag.cpu().numpy(),
                                                                   self._post.lam_off.cpu().numpy()))

    @property
    def posterior_covariance(self):
        if self._post is None:
            return None
        if self._post.P is None:     # computed on demand: P = R^T R (one MFMA GEMM)
            self._post = self.eng.posterior(self._dX, self.theta, self.kernel.__name__, self._dSigma_inv,
                                            self.eng.dev(self.fMAP), self.m, want_P=True)
        return self._lazy("P", lambda: self._post.P.cpu().numpy())

    @property
    def posterior_covariance_inv(self):
        if self._post is None:
            return None
        return self._lazy("Pinv", lambda: self.Sigma_inv - self.Lambda_MAP)

    def _dense_lambda(self, diag, off):
        N, mb = self.N, self.m + 1
        L = np.diag(diag)
        idx = np.arange(N)
        pse = idx[idx % mb != 0]
        obs = (pse // mb) * mb
        L[obs, pse] = off[pse]
        L[pse, obs] = off[pse]
        return L

    # ------------------------------------------------------------------ covariance
    def create_Gramian(self, X1, X2, kernel, *args):
        theta = args[0]
        return self.eng.gram(np.asarray(X1), theta, kernel.__name__, self.COVARIANCE_SHRINKAGE).cpu().numpy()

    def create_Gramian_nonsquare(self, X1, X2, kernel, *args):
        return kernel(X1, X2, *args)

    def update_Sigma(self, theta):
        self._dSigma = self.eng.gram(self._dX, theta, self.kernel.__name__, self.COVARIANCE_SHRINKAGE)
        self._invalidate("Sigma")
        self._drop_stale_factor(theta)

    def _drop_stale_factor(self, theta=None):
        """The Cholesky factor kept from update_Sigma_inv belongs to ONE (X, theta): once Sigma has been rebuilt for
        another theta or more rows, prior draws must not use it (an N_old x N_old factor against an
        N-vector, or the factor of the previous theta).  The incremental append keys on _sinv_state itself and is
        left alone: it checks theta and the row prefix before bordering."""
        st = self._sinv_state
        if self._dL is None:
            return
        th = None if theta is None else theta_key(theta)
        if st is None or self._dL.shape[0] != self.N or (th is not None and st[1] != th):
            self._dL_stale = True
        else:
            self._dL_stale = False

    def update_Sigma_inv(self, theta):
        th = theta_key(theta)
        st = self._sinv_state
        done = False
        if (self.incremental and st is not None and self._dLinv is not None and self._dL is not None and st[1] == th
                and st[2] < APPEND_REFRESH and 0 < self.N - st[0].shape[0] <= 64
                and np.array_equal(self.X[:st[0].shape[0]], st[0])):
            try:
                self._dSigma_inv, self._dLinv, self._dL = self.eng.pd_inverse_append(self._dSigma, self._dSigma_inv,
                                                                                       self._dLinv, self._dL)
                self._sinv_state = (self.X.copy(), th, st[2] + 1)
                self.n_appends += 1
                done = True
            except NotPositiveDefinite:
                pass                      # Schur complement lost definiteness to rounding: full inversion below
        if not done:
            # the Cholesky factor of Sigma comes with the inverse: the whitened f_MAP search and the prior draws use it
            if self.incremental:
                self._dSigma_inv, self._dLinv, self._dL = self.eng.pd_inverse_factors3(self._dSigma)
            else:
                (self._dSigma_inv, self._dL), self._dLinv = self.eng.pd_inverse_chol(self._dSigma), None
            self._sinv_state = (self.X.copy(), th, 0)
            self.n_full_inversions += 1
        self._dL_stale = False
        self._invalidate("Sigma_inv", "Pinv")

    def set_theta(self):
        self.theta = self.theta_initial
        if self.theta[1] is None:
            self.theta[1] = 1
        if self.theta[2] is None:
            self.theta[2] = 0.1
        if self.theta[0] is None:
            self.theta[0] = 8

    # ------------------------------------------------------------------ functional T
    def _sinv_dev(self, Sigma_inv_):
        return self._dSigma_inv if Sigma_inv_ is None else self.eng.dev(Sigma_inv_)

    def T(self, f, theta, Sigma_inv_=None):
        T, _ = self.eng.T_and_grad(self._sinv_dev(Sigma_inv_), np.asarray(f, dtype=float).ravel(), self.m, theta[0])
        return T

    def T_grad(self, f, theta, Sigma_inv_=None):
        _, g = self.eng.T_and_grad(self._sinv_dev(Sigma_inv_), np.asarray(f, dtype=float).ravel(), self.m, theta[0])
        return g.cpu().numpy()

    def create_Lambda(self, f, sigma):
        _, _, ld, lo = self.eng.laplace_terms(np.asarray(f, dtype=float).ravel(), self.m, sigma)
        return self._dense_lambda(ld.cpu().numpy(), lo.cpu().numpy())

    def T_hessian(self, f, theta, Sigma_inv_=None):
        Sinv = self.Sigma_inv if Sigma_inv_ is None else np.asarray(Sigma_inv_)
        return -Sinv + self.create_Lambda(f, theta[0])

    def sum_Phi_vec(self, order_of_derivative, f, sigma, over_all_indices=False):
        """gp_model.py:206-218 on the device (ppbo_sum_phi): one value per query, repeated over the query's m+1 rows
        when over_all_indices.  Order 0 is the closed form Phi(Delta/sqrt2) of the Gauss-Hermite integral at :192."""
        if order_of_derivative not in (0, 1, 2):
            print("The derivatives of an order higher than 2 are not needed!")
            return None
        out = self.eng.sum_phi(np.asarray(f, dtype=float).ravel(), self.m, sigma, order_of_derivative).cpu().numpy()
        return np.repeat(out, self.m + 1) if over_all_indices else out

    def sum_Phi(self, i, order_of_derivative, f, sigma, sample_points=None, weights=None):
        """gp_model.py:176-204: the sum for the query whose observation row is i (an element of obs_indices).  The
        quadrature arguments are accepted and unused (closed form)."""
        v = self.sum_Phi_vec(order_of_derivative, f, sigma)
        return None if v is None else float(v[int(i) // (self.m + 1)])

    # ------------------------------------------------------------------ concurrent fits
    def _side_engines(self, n):
        """n extra (Engine, stream) pairs on this model's GPU.  One f_MAP fit is a latency-bound chain of small
        launches that leaves most of the chip idle, so independent fits (evidence at different theta, the random
        restarts of the last iteration) run concurrently: one ppbo_ctx (private workspaces) and one HIP stream per
        host thread; ctypes releases the GIL inside every library call."""
        import torch
        from .engine import Engine
        pool = self.__dict__.setdefault("_side_pool", [])
        while len(pool) < n:
            pool.append((Engine(self.eng.device.index), torch.cuda.Stream(device=self.eng.device)))
        return pool[:n]

    def _run_concurrently(self, jobs, workers):
        """jobs: callables taking an Engine; returns their results in order.  workers <= 1: run on self.eng."""
        import queue
        import threading
        import torch
        if workers <= 1 or len(jobs) <= 1:
            return [job(self.eng) for job in jobs]
        side = self._side_engines(min(workers, len(jobs)))
        main = torch.cuda.current_stream(self.eng.device)
        todo = queue.Queue()
        for k, job in enumerate(jobs):
            todo.put((k, job))
        out, errs = [None] * len(jobs), []

        def worker(eng, stream):
            stream.wait_stream(main)                     # inputs were produced on the caller's stream
            with torch.cuda.stream(stream):
                while True:
                    try:
                        k, job = todo.get_nowait()
                    except queue.Empty:
                        break
                    try:
                        out[k] = job(eng)
                    except Exception as e:           # noqa: BLE001  (re-raised in the caller's thread)
                        errs.append(e)
                stream.synchronize()

        threads = [threading.Thread(target=worker, args=pair) for pair in side]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        if errs:
            raise errs[0]
        return out

    @staticmethod
    def _default_workers(N):
        # measured (tools/dev/r4_evidence_workers.py, 20 evidences): N = 512: 76.7 / 32.9 / 26.9 / 27.4 ms with 1 / 4 / 8 / 16
        # contexts; N = 2048: 214.7 / 86.5 / 76.7 / 67.9 ms -- beyond eight the host's launch rate is the limit
        return 8 if N <= 2048 else (4 if N <= 4096 else 2)

    # ------------------------------------------------------------------ evidence / hyper-parameters
    def _evidence_fit(self, eng, theta, f0, gtol=1e-4):
        """The Gram matrix, its inverse, f_MAP from f0 and Lambda(f_MAP) of one Laplace evidence on `eng`."""
        Sig = eng.gram(self._dX, theta, self.kernel.__name__, self.COVARIANCE_SHRINKAGE)
        if self.fMAP_method == "whitened":
            Sinv, L = eng.pd_inverse_chol(Sig)
        else:
            Sinv, L = eng.pd_inverse(Sig), None
        fm, st = eng.fit_fmap(Sinv, f0, self.m, theta[0], gtol=gtol, maxiter=500, L=L)
        _, _, ld, lo = eng.laplace_terms(fm, self.m, theta[0])
        return Sig, Sinv, fm, st, ld, lo

    def _prior_theta(self, theta):
        """theta as log_prior sees it: camphor_copper_ard_kernel's length scales always as the six l_d (a scalar expanded
        to the reference's profile), so that its prior is the sum over the six coordinates."""
        if self.kernel.__name__ == CAMPHOR_ARD:
            return [theta[0], lengthscales(theta, self.D, CAMPHOR_ARD), theta[2]]
        return theta

    def _evidence_core(self, eng, theta, f0):
        """One Laplace evidence on `eng` from the start vector f0 (device); returns (value incl. log-prior, log-evidence)."""
        Sig, _, _, st, ld, lo = self._evidence_fit(eng, theta, f0)
        sgn, logdet, _ = eng.laplace_logdet(Sig, ld, lo, self.m)
        log_evidence = st["T"] - 0.5 * sgn * logdet
        return log_evidence + log_prior(self._prior_theta(theta)), log_evidence

    def evidence(self, theta, f_initial):
        """Laplace log-marginal likelihood + log-prior (gp_model.py:278-319) on the device.
        As in the reference, f_initial is IGNORED and redrawn from N(0, self.Sigma) (:294), the matrix is
        I + Sigma_theta*Lambda_MAP (plus sign, :302) and the determinant term is the sum of sign*logdet over the
        LU factors (:307-310), i.e. sign(prod diag U) * sum log|diag U| with LAPACK's pivoting.  theta[1] may be a
        vector of per-dimension length scales (log_prior sums the length-scale prior over them)."""
        theta = _theta_list(theta)
        if self.verbose:
            print("---------- Iter results ----------------")
        value, log_evidence = self._evidence_core(self.eng, theta, self._draw_prior())
        if self.verbose:
            print("(scaled) Log-evidence: " + str(log_evidence))
            print("Hyper-parameters: " + str(theta))
        if np.isnan(value) or not np.isfinite(value):
            if self.verbose:
                print("Nan log-evidence!")
            return -500
        if self.verbose:
            print("(scaled) Log-evidence + Log-prior: " + str(value))
        return float(value)

    def evidence_batch(self, thetas, workers=None):
        """evidence() at many thetas: the start vectors are drawn first, in order, from the global stream (so the
        values equal those of sequential evidence() calls), then the independent fits run concurrently on this GPU;
        under torch.distributed (one process per GPU) rank r takes thetas[r::world] and ONE all-gather returns all
        values to every rank.  REQUIREMENT under torch.distributed: every rank calls this with the same thetas and
        an identically seeded global NumPy stream (the start vectors are drawn from it on every rank); a checksum
        of both is compared across ranks first and a mismatch raises.  NaN / inf -> -500 as in the reference
        (gp_model.py:314-316)."""
        from . import dist as _dist
        thetas = [_theta_list(th) for th in thetas]
        f0s = [self._draw_prior() for _ in thetas]
        rank, world = _dist.rank_world()
        if world > 1:
            # rank r evaluates thetas[r::world] and the values are merged BY POSITION: that is only meaningful when
            # every rank holds the same candidate list and the same start vectors, i.e. identical NumPy streams
            tarr = np.asarray([np.hstack([np.ravel(t) for t in th]) for th in thetas], dtype=float)
            _dist.assert_same_across_ranks(
                [len(thetas), float(tarr.sum()), float((tarr * np.arange(1, tarr.size + 1).reshape(tarr.shape)).sum()),
                 float(f0s[0].sum().item()) if f0s else 0.0],
                "evidence_batch: hyper-parameter candidates / start vectors", device=self.eng.device)
        mine = list(range(rank, len(thetas), world))
        workers = self._default_workers(self.N) if workers is None else workers
        jobs = [(lambda eng, k=k: self._evidence_core(eng, thetas[k], f0s[k])[0]) for k in mine]
        vals = self._run_concurrently(jobs, workers)
        vals = [(-500.0 if (v != v or not np.isfinite(v)) else float(v)) for v in vals]
        return _dist.allgather_strided(vals, len(thetas), device=self.eng.device)

    def optimize_theta(self, workers=None):
        """Evidence maximisation over (l, sigma_f) with sigma fixed to 1 (gp_model.py:391-413).  The reference
        drives GPyOpt's Bayesian optimisation (20 initial + 40 iterations = 60 evidence fits); GPyOpt is replaced
        by the same budget of device evidence fits: 20 uniform draws over the reference's box (one concurrent
        batch), then 4 batches of 10 shrinking Gaussian perturbations of the incumbent.  The search TRAJECTORY is
        unpinned (GPyOpt==1.2.6 absent); the objective is the pinned evidence().
        Per-dimension length scales in theta_initial: the same 2-parameter search, 60 evidence fits and box, over a common
        factor c of the initial profile, l = c p with p = l0 / geomean(l0), and sigma_f (fitting the D length scales
        one by one is optimize_theta_ard).  camphor_copper_ard_kernel always searches its profile, a scalar l standing for
        (l, l, l + 0.05, l, l, l)."""
        if self.verbose:
            print("Hyperparameter optimization begins...")
        start = time.time()
        l0 = self.theta_initial[1] if self.theta_initial is not None else None
        profile = None
        if l0 is not None and (np.ndim(l0) != 0 or self.kernel.__name__ == CAMPHOR_ARD):
            l0 = lengthscales(self.theta_initial, self.D, self.kernel.__name__)
            profile = l0 / np.exp(np.mean(np.log(l0)))

        def ls(c):
            return float(c) if profile is None else float(c) * profile
        lo, hi = np.array([0.01, 0.1]), np.array([2.0, 15.0])
        best_v, best_t = -np.inf, None
        self.theta_search_log = []
        for rnd in range(5):
            if rnd == 0:
                cands = lo + np.random.uniform(size=(20, 2)) * (hi - lo)
            else:
                width = 0.25 * (hi - lo) * (0.5 ** (rnd - 1))
                cands = np.clip(best_t + width * np.random.standard_normal((10, 2)), lo, hi)
            vals = self.evidence_batch([[1.0, ls(c[0]), c[1]] for c in cands], workers=workers)
            for c, v in zip(cands, vals):
                self.theta_search_log.append((float(c[0]), float(c[1]), float(v)))
                if v > best_v:
                    best_v, best_t = v, c
        if self.verbose:
            print("Optimization of hyperparameters took " + str(time.time() - start) + " seconds.")
        self.theta = [1.0, ls(best_t[0]), float(best_t[1])]
        if self.verbose:
            print("The optimized theta is " + str(self.theta))

    def evidence_grad(self, theta, f_initial=None, gtol=None):
        """evidence() and its gradient with respect to (l, sigma_f), sigma fixed (no reference counterpart).
        Returns (value, grad, log_evidence, s_U, f_MAP): value = log-evidence + log-prior as evidence() computes it (the
        same Gram, inverse, fit and LU; the start is f_initial, or a prior draw from the global stream when it is None,
        and f_MAP is found to gtol, default 1e-4 as in evidence()); grad has one entry per length scale (one for a
        scalar l, D for a vector) followed by dE/dsigma_f; s_U is the sign of the LU's prod u_kk, f_MAP the device
        vector; six for camphor_copper_ard_kernel, whose scalar l stands for its profile).  A non-finite value maps to
        -500 with a zero gradient.  Raises ValueError for the camphor-copper kernel and NotPositiveDefinite when Sigma or
        Sigma^-1 - Lambda(f_MAP) is not positive definite."""
        theta = _theta_list(theta)
        kern = self.kernel.__name__
        if kern not in ARD_KERNELS:
            raise ValueError(f"the evidence gradient is defined for the kernels {ARD_KERNELS}, not {kern}")
        ls = lengthscales(theta, self.D, kern)
        f0 = self._draw_prior() if f_initial is None else self.eng.dev(f_initial).reshape(-1)
        Sig, Sinv, fm, st, ld, lo = self._evidence_fit(self.eng, theta, f0, 1e-4 if gtol is None else float(gtol))
        sgn, logdet, sums, _ = self.eng.evidence_grad(self._dX, theta, kern, Sig, Sinv, fm, ld, lo, self.m,
                                                      self.COVARIANCE_SHRINKAGE)
        log_evidence = st["T"] - 0.5 * sgn * logdet
        value = log_evidence + log_prior(self._prior_theta(theta))
        sf = theta[2]
        # dSigma_ij/dl_d = -2 (1 - eps) sf^2 kappa'(rho^2) (x_id - x_jd)^2 / (l_dev^2 l_d), l_dev = 1 for ARD rows
        coef = -2.0 * (1.0 - self.COVARIANCE_SHRINKAGE) * sf * sf
        raw = sums[:-1]
        if kern == CAMPHOR_ARD:
            raw = camphor_coordinate_sums(raw)
            theta = self._prior_theta(theta)
        if ls is None:
            gl = np.array([coef * float(np.sum(raw)) / theta[1] ** 3])
        else:
            gl = coef * raw / ls
        grad = np.append(gl, 2.0 * sums[-1] / sf) + log_prior_grad(theta)
        if not np.isfinite(value) or not np.all(np.isfinite(grad)):
            return -500.0, np.zeros_like(grad), log_evidence, sgn, fm
        return float(value), grad, log_evidence, sgn, fm

    def optimize_theta_ard(self, maxfun=60, start=None):
        """Evidence maximisation over one length scale per input dimension and sigma_f, sigma fixed to 1 (no reference
        counterpart; GPy / scikit-learn's ARD fit).  L-BFGS-B over (log l_1..log l_D, log sigma_f) with evidence_grad's
        device gradient, inside the reference's box (l_d in [0.01, 2], sigma_f in [0.1, 15]).  Starts from `start` (a
        theta; a scalar l is broadcast to D) or the current theta.  Each evaluation's f_MAP search starts at the previous
        evaluation's f_MAP; the first at the model's f_MAP when it has N rows, else at one prior draw from the global
        stream.  At most `maxfun` evidence fits, every one logged in theta_search_log as (l, sigma_f, value); theta
        becomes the best one seen, so never a worse one than the start.  camphor_copper_ard_kernel: a scalar l in the
        start is expanded to its profile (l, l, l + 0.05, l, l, l)."""
        kern = self.kernel.__name__
        if kern not in ARD_KERNELS:
            raise ValueError(f"per-dimension length scales are fitted for the kernels {ARD_KERNELS}, not {kern}")
        if self.verbose:
            print("Hyperparameter optimization (ARD, evidence gradient) begins...")
        t0 = time.time()
        if start is None:
            if self.theta is None:
                self.set_theta()
            start = self.theta
        start = _theta_list(start)
        l0 = lengthscales(start, self.D, kern)
        l0 = np.full(self.D, float(start[1])) if l0 is None else l0
        D = self.D
        (llo, lhi), (slo, shi) = THETA_BOX
        lo = np.log(np.append(np.full(D, llo), slo))
        hi = np.log(np.append(np.full(D, lhi), shi))
        p0 = np.clip(np.log(np.append(l0, float(start[2]))), lo, hi)
        if self.fMAP is not None and len(self.fMAP) == self.N:
            f_state = [self.eng.dev(self.fMAP)]
        else:
            f_state = [self._draw_prior()]
        best = {"v": -np.inf, "p": p0}
        self.theta_search_log = []

        class _Budget(Exception):
            pass

        def fg(p):
            if len(self.theta_search_log) >= maxfun:
                raise _Budget()
            p = np.clip(np.asarray(p, dtype=float), lo, hi)
            q = np.exp(p)
            theta = [1.0, q[:D].copy(), float(q[D])]
            try:
                v, g, _, _, fm = self.evidence_grad(theta, f_initial=f_state[0], gtol=ARD_FIT_GTOL)
                if v != -500.0:
                    f_state[0] = fm
            except NotPositiveDefinite:
                v, g = -500.0, np.zeros(D + 1)
            self.theta_search_log.append((q[:D].copy(), float(q[D]), float(v)))
            if v > best["v"]:
                best["v"], best["p"] = v, p.copy()
            return -v, -(g * q)                   # d/dlog x = x d/dx

        try:
            scipy.optimize.minimize(fg, p0, jac=True, method="L-BFGS-B", bounds=list(zip(lo, hi)),
                                    options=dict(maxfun=maxfun, maxiter=maxfun))
        except _Budget:
            pass
        q = np.exp(best["p"])
        self.theta = [1.0, q[:D].copy(), float(q[D])]
        if self.verbose:
            print("Optimization of hyperparameters took " + str(time.time() - t0) + " seconds.")
            print("The optimized theta is " + str(self.theta))

    # ------------------------------------------------------------------ f_MAP
    def _draw_prior(self):
        """f ~ N(0, Sigma) for the random start (gp_model.py:374,381): L z with the device Cholesky
        factor and z from the global NumPy stream (the reference uses np.random.multivariate_normal)."""
        if self._dL is not None and not self.__dict__.get("_dL_stale", False) and self._dL.shape[0] == self.N:
            # factor of the current Sigma, from update_Sigma_inv
            return self.eng.dgemv(self._dL, np.random.standard_normal(self.N), lower=True)
        key = (self._dSigma.data_ptr(), getattr(self._dSigma, "_version", 0))
        cache = self.__dict__.get("_prior_chol")
        if cache is None or cache[0] != key:
            cache = (key, self.eng.potrf_(self._dSigma.clone()), self._dSigma)     # keeps Sigma alive: the pointer stays unique
            self._prior_chol = cache
        return self.eng.dgemv(cache[1], np.random.standard_normal(self.N), lower=True)

    def update_fMAP(self, random_initial_vector=None, fmap_finding_trials=None, approx_optimization=False):
        trials = self.fMAP_finding_trials if fmap_finding_trials is None else fmap_finding_trials
        rnd = self.fMAP_random_initial_vector if random_initial_vector is None else random_initial_vector
        gtol = 100.0 if approx_optimization else self.fMAP_gtol   # gp_model.py:365-368 (SciPy default gtol 1e-4)
        if self.verbose:
            print("MAP-estimation begins...")
        start = time.time()
        best_T, best = -np.inf, None
        # incremental mode: one warm start replaces the reference's default prior draw (not on the last
        # iteration, whose 10 random restarts are the reference's guard against local optima, gp_model.py:96-97)
        warm = (self.incremental and self.fMAP is not None and len(self.fMAP) <= self.N and not self.last_iteration
                and random_initial_vector is None and fmap_finding_trials is None)
        if warm:
            rnd, trials = False, 1
        starts = []
        for _ in range(trials):
            if self.fMAP is None or rnd or len(self.fMAP) > self.N:
                f0 = self._draw_prior()
            elif len(self.fMAP) < self.N:
                n_old = len(self.fMAP)
                pm = self._post_mean
                if warm and pm is not None and pm.X.shape[0] == n_old:
                    # previous posterior mean at the appended rows: K(X_new, X_old) alpha_old
                    pad = self.eng.predict(pm, self.X[n_old:], score=SCORE_MEAN, want_var=False,
                                           want_best=False)["mu"].cpu().numpy()
                else:                                            # pad with the mean (gp_model.py:375-377)
                    pad = np.full(self.N - n_old, np.mean(self.fMAP))
                f0 = np.concatenate([self.fMAP, pad])
            else:
                f0 = self.fMAP
            starts.append(self.eng.dev(f0))
        # independent restarts (the reference's 10 on the last iteration, gp_model.py:96-97) run concurrently
        t_fit = time.time()
        L = self._dL if self.fMAP_method == "whitened" else None
        jobs = [(lambda eng, f0=f0: eng.fit_fmap(self._dSigma_inv, f0, self.m, self.theta[0], gtol=gtol, L=L))
                for f0 in starts]
        results = self._run_concurrently(jobs, self._default_workers(self.N) if trials > 1 else 1)
        t_fit = (time.time() - t_fit) / max(trials, 1)
        for fm, st in results:
            if trials > 1:               # produced on a side stream, consumed on the caller's from here on
                import torch
                fm.record_stream(torch.cuda.current_stream(self.eng.device))
            self.fit_log.append(dict(N=self.N, method=self.fMAP_method, iterations=st["iterations"], n_cholesky=st["n_cholesky"],
                                     lbfgs_evals=st.get("lbfgs_evals", 0), lbfgs_status=st.get("lbfgs_status", -1),
                                     converged=st["converged"], warm=bool(warm), seconds=t_fit))
            if (self.fMAP_restart_on_stall and not st["converged"] and not approx_optimization
                    and st["gradnorm"] > 1e3 * gtol):
                # opt-in (off by default: it draws from the global NumPy stream, which would shift every later
                # design relative to the reference's trace).  The trust region stalled far from stationarity (no
                # descent predicted / radius collapsed): the reference hands back SciPy's last iterate
                # (gp_model.py:382-389); with the flag set, one fresh start from the prior is tried as well
                print("---!!!--- f_MAP search stopped at |grad T| = " + str(st["gradnorm"]) + "; restarting from a prior draw")
                fm2, st2 = self.eng.fit_fmap(self._dSigma_inv, self._draw_prior(), self.m, self.theta[0], gtol=gtol, L=L)
                if st2["T"] > st["T"] or not np.isfinite(st["T"]):
                    fm, st = fm2, st2
            if self.verbose:
                print("... this took " + str(time.time() - start) + " seconds.")
            if st["T"] > best_T:
                best_T, best, self.fit_stats = st["T"], fm, st
        if best is None:        # every trial ended with a non-finite T: keep the previous estimate, like a failed minimize
            print("---!!!--- f_MAP search produced no finite objective; keeping the previous f_MAP ---!!!---")
            if self.fMAP is None or len(self.fMAP) != self.N:
                self.fMAP = np.zeros(self.N)
            best = self.eng.dev(self.fMAP)
        self.fMAP = best.cpu().numpy()
        # like the reference, the previous Lambda_MAP / posterior covariance stay in place until
        # update_model recomputes them (and survive a failed recomputation, gp_model.py:115-120)
        self._refresh_mean_state(best)

    def _refresh_mean_state(self, fmap_dev):
        alpha = self.eng.dgemv(self._dSigma_inv, fmap_dev)
        self._post_mean = self.eng.mean_posterior(self._dX, self.theta, self.kernel.__name__, self.m, alpha)

    def _fit_fused(self, defer_posterior=False):
        """The default update (one prior-draw start, whitened search) as ONE library call: ppbo_gp_fit builds Sigma,
        its factor and inverse, runs the search from the prior draw L z0 -- z0 from the global NumPy stream, exactly the
        numbers _draw_prior would have consumed -- and the posterior state, with one host wait instead of one per
        phase (update_Sigma + update_Sigma_inv + update_fMAP + the posterior of src/gp_model.py:91-117).
        Returns False (nothing done) when the configuration needs the call-by-call path."""
        if (self.incremental or self.fMAP_method != "whitened" or self.last_iteration or self.fMAP_finding_trials != 1
                or not self.fMAP_random_initial_vector or self.fMAP_restart_on_stall):
            return False
        if self.verbose:
            print("MAP-estimation begins...")
        start = time.time()
        z0 = np.random.standard_normal(self.N)
        # defer_posterior (update_model, N >= 1024): the call ends with f_MAP; Lambda_MAP / the posterior factor -- a
        # latency-bound chain of 0.9 ms at N = 2048 that mu_star does not need (it reads alpha only) -- then run on a second
        # ctx and stream BESIDE mu_star (_start_posterior / _finish_posterior): update_model at C3 3.9 -> 3.5 ms
        r = self.eng.gp_fit(self._dX, self.theta, self.kernel.__name__, self.m, z0, shrink=self.COVARIANCE_SHRINKAGE,
                            gtol=self.fMAP_gtol, start_is_whitened=True, want_Sigma=True,
                            want_posterior=not defer_posterior)
        th = theta_key(self.theta)
        self._dSigma, self._dSigma_inv, self._dL, self._dLinv = r["Sigma"], r["Sigma_inv"], r["L"], None
        self._sinv_state = (self.X.copy(), th, 0)
        self._dL_stale = False
        self.n_full_inversions += 1
        self._invalidate("Sigma", "Sigma_inv", "Pinv")
        st = r["stats"]
        self.fit_stats = st
        self.fit_log.append(dict(N=self.N, method="whitened (ppbo_gp_fit)", iterations=st["iterations"],
                                 n_cholesky=st["n_cholesky"], lbfgs_evals=st["lbfgs_evals"],
                                 lbfgs_status=st["lbfgs_status"], converged=st["converged"], warm=False,
                                 seconds=time.time() - start))
        fm_host = r["fMAP"].cpu().numpy()
        if not (np.isfinite(st["T"]) and np.all(np.isfinite(fm_host))):
            # neither the search nor the finisher behind it (lbfgs_status 4 = the start had no finite objective; the
            # trust region may still have recovered one: then T and f_MAP ARE finite and the fit stands) produced a finite
            # objective: what update_fMAP does when every trial ends that way -- the previous estimate stays.  Mean AND
            # variance state are rebuilt from it at the CURRENT design, so that next_query never mixes a new mean with a
            # posterior of another N
            print("---!!!--- f_MAP search produced no finite objective; keeping the previous f_MAP ---!!!---")
            if self.fMAP is None or len(self.fMAP) != self.N:
                self.fMAP = np.zeros(self.N)
            kept = self.eng.dev(self.fMAP)
            self._refresh_mean_state(kept)
            try:
                self._post = self._post_mean = self.eng.posterior(self._dX, self.theta, self.kernel.__name__,
                                                                  self._dSigma_inv, kept, self.m, want_P=False)
                self._invalidate("Lambda_MAP", "P", "Pinv")
            except NotPositiveDefinite:
                print("---!!!--- Posterior covariance matrix is not PSD ---!!!---")
                if self._post is not None and self._post.X.shape[0] != self.N:
                    self._post = None      # a posterior of another design: predictions of the variance raise instead
                    self._invalidate("Lambda_MAP", "P", "Pinv")
            return True
        self.fMAP = fm_host
        if self.verbose:
            print("... this took " + str(time.time() - start) + " seconds.")
            print("Current theta is: " + str(self.theta) + " (Acq. = " + str(self.xi_acquisition_function) + ")")
            print("Updating Lambda_MAP and posterior covariance...")
        if defer_posterior:
            self._refresh_mean_state(r["fMAP"])            # alpha: all mu_star needs
            self._start_posterior(r["fMAP"])
        elif r["post"] is not None:
            self._post = self._post_mean = r["post"]
            self._invalidate("Lambda_MAP", "P", "Pinv")
        else:
            print("---!!!--- Posterior covariance matrix is not PSD ---!!!---")   # gp_model.py:119, keep the old one
            self._refresh_mean_state(r["fMAP"])
        return True

    def _start_posterior(self, fmap_dev):
        """Lambda_MAP, alpha and the posterior factor G (ppbo_posterior) on a side ctx / stream, in a host thread of its
        own (the call ends with a host wait; ctypes releases the GIL): the caller goes on with mu_star and collects the
        result with _finish_posterior."""
        import threading
        import torch
        (side, stream), = self._side_engines(1)
        box = {}
        main = torch.cuda.current_stream(self.eng.device)

        # f_MAP and Sigma^-1 were produced on the caller's stream: the dependency is recorded HERE, in the calling thread,
        # before mu_star enqueues anything on `main` -- recorded inside the worker it would land wherever `main` happens to
        # be when that thread first runs, and the side stream would then wait for mu_star's launches as well
        stream.wait_stream(main)

        def work():
            try:
                with torch.cuda.stream(stream):
                    box["post"] = side.posterior(self._dX, self.theta, self.kernel.__name__, self._dSigma_inv, fmap_dev,
                                                 self.m, want_P=False)
                    stream.synchronize()
            except Exception as e:                      # noqa: BLE001  (looked at in _finish_posterior)
                box["err"] = e

        th = threading.Thread(target=work)
        th.start()
        self._pending_posterior = (th, box)

    def _finish_posterior(self):
        pend = self.__dict__.pop("_pending_posterior", None)
        if pend is None:
            return
        import torch
        th, box = pend
        th.join()
        err = box.get("err")
        if isinstance(err, NotPositiveDefinite):
            print("---!!!--- Posterior covariance matrix is not PSD ---!!!---")   # gp_model.py:119, keep the old one
            return
        if err is not None:
            raise err
        post = box["post"]
        main = torch.cuda.current_stream(self.eng.device)
        for t in (post.alpha, post.lam_diag, post.lam_off, post.G):
            t.record_stream(main)                       # allocated on the side stream, consumed on the caller's from here on
        self._post = self._post_mean = post
        self._invalidate("Lambda_MAP", "P", "Pinv")

    # ------------------------------------------------------------------ orchestration (gp_model.py:87-132)
    def update_model(self, optimize_theta=False):
        if self.theta is None:
            self.set_theta()
        init_skip = self.initialization_running and self.skip_computations_during_initialization
        fused = (not init_skip) and (not optimize_theta) and self._fit_fused(defer_posterior=self.N >= 1024)
        if not fused:
            self.update_Sigma(self.theta)
            self.update_Sigma_inv(self.theta)
            if init_skip:
                self.FP.alpha_grid_distribution = "equispaced"
                self.update_fMAP(random_initial_vector=False, fmap_finding_trials=1, approx_optimization=True)
            elif self.last_iteration:
                self.update_fMAP(random_initial_vector=True, fmap_finding_trials=10)
            else:
                self.update_fMAP()
            if optimize_theta:
                if self.theta_optimizer == "ard-gradient":
                    self.optimize_theta_ard()
                else:
                    self.optimize_theta()
                self.update_fMAP()
                self.update_Sigma(self.theta)
                self.update_Sigma_inv(self.theta)
            if self.verbose:
                print("Current theta is: " + str(self.theta) + " (Acq. = " + str(self.xi_acquisition_function) + ")")
            if not init_skip:
                if self.verbose:
                    print("Updating Lambda_MAP and posterior covariance...")
                start = time.time()
                if self.N >= 1024 and not self.last_iteration:
                    # beside mu_star, as after the fused fit (the restarts of the last iteration occupy the side contexts)
                    self._start_posterior(self.eng.dev(self.fMAP))
                else:
                    try:
                        self._post = self.eng.posterior(self._dX, self.theta, self.kernel.__name__, self._dSigma_inv,
                                                        self.eng.dev(self.fMAP), self.m, want_P=False)
                        self._post_mean = self._post
                        self._invalidate("Lambda_MAP", "P", "Pinv")
                    except NotPositiveDefinite:
                        print("---!!!--- Posterior covariance matrix is not PSD ---!!!---")   # gp_model.py:119, keep the old one
                if self.verbose:
                    print("... this took " + str(time.time() - start) + " seconds.")
        if self.verbose:
            print("Computing mu_star and x_star ...")
        start = time.time()
        try:
            if init_skip and not self.skip_xstaroptimization_during_initialization:
                self.xstar, self.mustar, self.xstars_local = self.mu_star(mustar_finding_trials=1)
            elif self.initialization_running and self.skip_xstaroptimization_during_initialization:
                pass
            elif self.last_iteration:
                self.xstar, self.mustar, self.xstars_local = self.mu_star(mustar_finding_trials=20)
            else:
                self.xstar, self.mustar, self.xstars_local = self.mu_star()
        finally:
            self._finish_posterior()                   # the posterior factor that ran beside mu_star (if any)
        if self.verbose:
            print("... this took " + str(time.time() - start) + " seconds.")

    # ------------------------------------------------------------------ predictions
    def _mean_post(self):
        if self._post_mean is None:
            raise RuntimeError("update_model()/update_fMAP() must run before predictions")
        return self._post_mean

    def _var_post(self):
        """The posterior with its variance operator, which every prediction beyond the mean needs."""
        if self._post is None or self._post.G is None:
            raise RuntimeError("posterior covariance unavailable (skipped during initialisation, gp_model.py:106-107)")
        return self._post

    def mu_Sigma_pred(self, X_pred):
        post = self._var_post()
        mu, cov = self.eng.predict_cov(post, np.atleast_2d(X_pred), self.COVARIANCE_SHRINKAGE)
        return mu.cpu().numpy(), cov.cpu().numpy()

    def preference_pred(self, Xa, Xb):
        """(mu_d, var_d, p) as NumPy arrays for the duels (Xa[i], Xb[i]): the posterior mean and variance of
        f(a) - f(b) and p = P(a > b) = Phi(mu_d / sqrt(2 sigma^2 + var_d)) (ppbo_predict_pairs; no reference
        counterpart).  Host or device input; one pair may be given as two 1-D vectors."""
        post = self._var_post()
        Xa, Xb = (x if x.dim() == 2 else x.reshape(1, -1) for x in (self.eng.dev(Xa), self.eng.dev(Xb)))
        out = self.eng.predict_pairs(post, Xa, Xb, want_best=False)
        return out["mu"].cpu().numpy(), out["var"].cpu().numpy(), out["prob"].cpu().numpy()

    def slope_pred(self, X, Xi):
        """(mu_s, var_s, p) as NumPy arrays for the rows (X[i], Xi[i]): the posterior mean and variance of the slope
        d/da f(x + a xi) at a = 0 and p = P(slope > 0) = Phi(mu_s / sqrt(var_s)), without a noise term
        (ppbo_predict_slopes; no reference counterpart).  Host or device input in the caller's coordinates; one row may
        be given as two 1-D vectors.  ValueError when the two shapes differ or do not fit the model."""
        post = self._var_post()
        X, Xi = (a if isinstance(a, torch.Tensor) else np.asarray(a, dtype=float) for a in (X, Xi))
        X, Xi = (a.reshape(1, -1) if a.ndim == 1 else a for a in (X, Xi))
        out = self.eng.predict_slopes(post, X, Xi, want_best=False)
        return out["mu"].cpu().numpy(), out["var"].cpu().numpy(), out["prob"].cpu().numpy()

    def sensitivity(self, x=None):
        """The D coordinate slopes at x (default: xstar) as three length-D NumPy arrays (mu_s, var_s, p): row d is
        slope_pred(x, e_d).  p near 1/2 with a small |mu_s|: the parameter is locally settled; p near 0 or 1: the
        model expects the utility to change along it."""
        x = np.asarray(self.xstar if x is None else x, dtype=float).reshape(-1)
        return self.slope_pred(np.tile(x, (x.size, 1)), np.eye(x.size))

    def curvature_pred(self, X, Xi):
        """(mu_c, var_c, p) as NumPy arrays for the rows (X[i], Xi[i]): the posterior mean and variance of the curvature
        d^2/da^2 f(x + a xi) at a = 0 and p = P(curvature < 0) = Phi(-mu_c / sqrt(var_c)), without a noise term
        (ppbo_predict_curvatures; no reference counterpart).  Input conventions and errors as slope_pred; a Matern-3/2
        model is refused with a ValueError (the curvature of its sample paths has no finite variance)."""
        post = self._var_post()
        X, Xi = (a if isinstance(a, torch.Tensor) else np.asarray(a, dtype=float) for a in (X, Xi))
        X, Xi = (a.reshape(1, -1) if a.ndim == 1 else a for a in (X, Xi))
        out = self.eng.predict_curvatures(post, X, Xi, want_best=False)
        return out["mu"].cpu().numpy(), out["var"].cpu().numpy(), out["prob"].cpu().numpy()

    def sharpness(self, x=None):
        """The D coordinate curvatures at x (default: xstar, where sensitivity() reads "settled" by construction) as three
        length-D NumPy arrays (mu_c, var_c, p): row d is curvature_pred(x, e_d).  p near 1 with a large |mu_c|: a
        confirmed, sharp peak in that parameter; p near 1/2: the model cannot tell a peak from a plateau there."""
        x = np.asarray(self.xstar if x is None else x, dtype=float).reshape(-1)
        return self.curvature_pred(np.tile(x, (x.size, 1)), np.eye(x.size))

    def functional_pred(self, X_groups, weights, threshold=0.0):
        """(mu, var, p) as NumPy arrays for the groups X_groups[i] ([M, G, D], or one group [G, D]) and the weights
        ([G]: one row for all groups, or [M, G]): the posterior mean and variance of L f = sum_g w_g f(x_g) and
        p = P(L f > threshold) = Phi((mu - threshold) / sqrt(var)), without a noise term (ppbo_predict_functionals; no
        reference counterpart).  Host or device input in the caller's coordinates, mapped as preference_pred maps its
        sides.  ValueError when the shapes do not fit each other or the model, or G > 64."""
        post = self._var_post()
        Xg, w = (a if isinstance(a, torch.Tensor) else np.asarray(a, dtype=float) for a in (X_groups, weights))
        if Xg.ndim == 2:
            Xg = Xg.reshape(1, *Xg.shape)
        out = self.eng.predict_functionals(post, Xg, w, threshold=threshold, want_best=False)
        return out["mu"].cpu().numpy(), out["var"].cpu().numpy(), out["prob"].cpu().numpy()

    def marginal_pred(self, dims, t, effect="centred"):
        """(mu, var, p) as NumPy arrays of f with every coordinate but the kept ones averaged over the unit box
        (ppbo_predict_marginals; no reference counterpart).  Row i keeps the 0-based axes dims[i] ([M, 2] with -1 = unused,
        or one-dimensional [M] for ONE axis per row whatever M is: a single order-2 row is [[d, e]]) at the values t[i]; effect: "raw" the marginal itself, "centred" (default) minus the
        overall mean of f, "interaction" the pure interaction f_de - f_d - f_e + fbar; p = P(effect > 0), without a
        noise term.  A utility learned from preferences is defined up to a constant, so "centred" and "interaction"
        are the identifiable quantities.  Closed form for SE_kernel (scalar or per-dimension length scales) and the
        camphor-copper kernels; ValueError for RQ and the Matern kernels (average_pred samples the box instead) and for
        rows that break the rules."""
        post = self._var_post()
        out = self.eng.predict_marginals(post, dims, t, effect=effect, want_best=False)
        return out["mu"].cpu().numpy(), out["var"].cpu().numpy(), out["prob"].cpu().numpy()

    @staticmethod
    def _effect_grid(grid, default=65):
        g = np.linspace(0.0, 1.0, default) if grid is None else np.asarray(grid, dtype=float).reshape(-1)
        if g.size < 1:
            raise ValueError("an effect needs at least one grid point")
        return g

    def main_effect(self, d, grid=None):
        """(grid, mu, var, p) of the centred main effect of coordinate d (0-based, as the rows of sensitivity()): how the
        utility depends on x_d once every other coordinate is averaged out, relative to the overall mean.  Default
        grid: 65 equispaced points of [0, 1]."""
        g = self._effect_grid(grid)
        mu, var, p = self.marginal_pred(np.full((g.size, 1), int(d)), g.reshape(-1, 1), effect="centred")
        return g, mu, var, p

    def interaction_effect(self, d, e, grid_d=None, grid_e=None, pure=True):
        """(mu, var, p) as [T_d, T_e] arrays over grid_d x grid_e (default 65 equispaced points each) of the interaction of
        the coordinates d and e: pure=True the pure interaction f_de - f_d - f_e + fbar (zero where the two act
        additively), pure=False the centred two-dimensional marginal f_de - fbar."""
        gd, ge = self._effect_grid(grid_d), self._effect_grid(grid_e)
        dims = np.tile(np.array([[int(d), int(e)]]), (gd.size * ge.size, 1))
        t = np.stack(np.meshgrid(gd, ge, indexing="ij"), axis=-1).reshape(-1, 2)
        mu, var, p = self.marginal_pred(dims, t, effect="interaction" if pure else "centred")
        return tuple(a.reshape(gd.size, ge.size) for a in (mu, var, p))

    def effect_importance(self, T=33):
        """The global companion of sensitivity(): which coordinates matter over the whole box, and which pairs interact.
        Returns a dict with, per axis, `main_range` [D] (max - min of the centred main-effect mean over T equispaced
        points), `main_argmax` [D] (its maximiser) and `main_sd` [D] (the largest posterior sd on the grid), and per
        pair d < e `pairs` [D (D - 1) / 2, 2] with `interaction_max` (the largest |mu| of the pure interaction on the
        T x T grid).  All D main-effect maps come from ONE predict_marginals call, all pair maps from one more."""
        post = self._var_post()
        D = int(self.D)
        g = self._effect_grid(None, int(T))
        T = g.size
        dims = np.repeat(np.arange(D), T)
        out = self.eng.predict_marginals(post, dims.reshape(-1, 1), np.tile(g, D).reshape(-1, 1), effect="centred",
                                         want_prob=False, kind=PAIR_MEAN, want_best=False)
        mu = out["mu"].cpu().numpy().reshape(D, T)
        sd = np.sqrt(np.maximum(out["var"].cpu().numpy().reshape(D, T), 0.0))
        res = dict(grid=g, main_range=mu.max(axis=1) - mu.min(axis=1), main_argmax=g[mu.argmax(axis=1)],
                   main_sd=sd.max(axis=1), pairs=np.zeros((0, 2), dtype=int), interaction_max=np.zeros(0))
        pairs = np.array([(d, e) for d in range(D) for e in range(d + 1, D)], dtype=int).reshape(-1, 2)
        if len(pairs):
            tt = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
            out = self.eng.predict_marginals(post, np.repeat(pairs, T * T, axis=0), np.tile(tt, (len(pairs), 1)),
                                             effect="interaction", want_var=False, want_prob=False, kind=PAIR_MEAN,
                                             want_best=False)
            res["pairs"] = pairs
            res["interaction_max"] = np.abs(out["mu"].cpu().numpy().reshape(len(pairs), T * T)).max(axis=1)
        return res

    def _neighbourhoods(self, X, offsets):
        """[M, G, D] clouds x + delta_g in the caller's coordinates, clipped to the box; the periodic coordinates of the
        camphor kernels (all but the third) are left as they are: the kernel is periodic there."""
        X = np.atleast_2d(np.asarray(X.cpu() if isinstance(X, torch.Tensor) else X, dtype=float))
        off = np.atleast_2d(np.asarray(offsets.cpu() if isinstance(offsets, torch.Tensor) else offsets, dtype=float))
        if X.shape[1] != self.D or off.shape[1] != self.D:
            raise ValueError(f"points of shape {X.shape} and offsets of shape {off.shape} for a model of {self.D} dimensions")
        Xg = X[:, None, :] + off[None, :, :]
        lo = np.array([b[0] for b in self.bounds], dtype=float)
        hi = np.array([b[1] for b in self.bounds], dtype=float)
        clipped = np.clip(Xg, lo, hi)
        if "camphor" in self.kernel.__name__:
            periodic = np.arange(self.D) != 2
            clipped[..., periodic] = Xg[..., periodic]
        return clipped

    def average_pred(self, X, offsets):
        """(mu, var) as NumPy arrays of the neighbourhood average (1 / G) sum_g f(x + delta_g) at the rows of X [M, D] for
        the shared offsets delta [G, D]: the expected utility of a design under implementation tolerance.  Offsets are
        added in the caller's coordinates and clipped to the box (not the periodic coordinates of the camphor kernels)."""
        Xg = self._neighbourhoods(X, offsets)
        G = Xg.shape[1]
        mu, var, _ = self.functional_pred(Xg, np.full(G, 1.0 / G))
        return mu, var

    def contrast_pred(self, XA, XB):
        """(mu, var, p) of mean_{a in A} f(a) - mean_{b in B} f(b) for two shortlists XA [GA, D], XB [GB, D]
        (GA + GB <= 64) with p = P(A is better on average); [M, GA, D] and [M, GB, D] give M contrasts."""
        A, B = (a if isinstance(a, torch.Tensor) else np.asarray(a, dtype=float) for a in (XA, XB))
        A, B = (a.reshape(1, -1) if a.ndim == 1 else a for a in (A, B))
        if A.ndim != B.ndim or A.ndim not in (2, 3) or (A.ndim == 3 and A.shape[0] != B.shape[0]):
            raise ValueError(f"contrast_pred: shortlists of shapes {tuple(A.shape)} and {tuple(B.shape)}")
        ga, gb = A.shape[-2], B.shape[-2]
        if ga + gb > 64:
            raise ValueError(f"contrast_pred: {ga} + {gb} points (at most 64 together)")
        Xg = torch.cat([self.eng.dev(A), self.eng.dev(B)], dim=-2)
        w = np.concatenate([np.full(ga, 1.0 / ga), np.full(gb, -1.0 / gb)])
        return self.functional_pred(Xg, w)

    def robust_xstar(self, offsets):
        """(x, mu_avg, var_avg): the row that maximises the neighbourhood-averaged posterior mean
        (1 / G) sum_g mu(x + delta_g) over the resident candidate pool and xstars_local, through the entry's score and
        argmax -- the robust optimum in place of the sharp one -- with the mean and variance of that average."""
        post = self._var_post()
        cand = self._candidate_pool().cpu().numpy()
        if self.xstars_local is not None and len(self.xstars_local):
            cand = np.concatenate([cand, np.atleast_2d(np.asarray(self.xstars_local, dtype=float))])
        Xg = self._neighbourhoods(cand, offsets)
        G = Xg.shape[1]
        out = self.eng.predict_functionals(post, Xg, np.full(G, 1.0 / G), score=0, want_prob=False)
        i = int(out["best_idx"])
        if i < 0:
            raise RuntimeError("robust_xstar: no candidate has a finite averaged mean")
        return cand[i].copy(), float(out["mu"][i]), float(out["var"][i])

    def mean_hessian(self, x=None):
        """The symmetric D x D Hessian of the posterior mean at x (default: xstar), by polarisation from the D (D + 1) / 2
        mean curvatures along e_a and e_a + e_b: H_ab = (mu_c(e_a + e_b) - mu_c(e_a) - mu_c(e_b)) / 2.  Needs no variance
        operator (a posterior without G serves; no posterior at all is _var_post's error).  Its eigenvalues tell a peak
        from a ridge or a saddle."""
        post = self._post if getattr(self, "_post", None) is not None else self._var_post()
        x = np.asarray(self.xstar if x is None else x, dtype=float).reshape(-1)
        D = x.size
        ia, ib = np.triu_indices(D)
        E = np.eye(D)
        Xi = np.where((ia == ib)[:, None], E[ia], E[ia] + E[ib])
        mu = self.eng.predict_curvatures(post, np.tile(x, (ia.size, 1)), Xi, score=0, want_var=False, want_prob=False,
                                         want_best=False)["mu"].cpu().numpy()
        H = np.zeros((D, D))
        diag = mu[ia == ib]
        H[ia, ib] = np.where(ia == ib, mu, 0.5 * (mu - diag[ia] - diag[ib]))
        H[ib, ia] = H[ia, ib]
        return H

    def gradient_pred(self, X):
        """(mean [M, D], cov [M, D, D]) as NumPy arrays: the posterior of the whole gradient, grad f(X[i]) ~ N(mean[i],
        cov[i]), in the caller's coordinates (ppbo_predict_gradients; no reference counterpart).  slope_pred's numbers are
        its projections: xi' mean and xi' cov xi.  Host or device input; one point may be given as a 1-D vector."""
        post = self._var_post()
        X = X if isinstance(X, torch.Tensor) else np.asarray(X, dtype=float)
        X = X.reshape(1, -1) if X.ndim == 1 else X
        out = self.eng.predict_gradients(post, X, want_best=False)
        return out["mean"].cpu().numpy(), out["cov"].cpu().numpy()

    def xstar_covariance(self, x=None):
        """How well the optimum is located: by the delta method x* ~ N(x, H^-1 C H^-1) at the peak x of the posterior
        mean (default: xstar), H = mean_hessian(x) and grad f(x) ~ N(m, C) from gradient_pred.  Returns dict(cov, hessian,
        grad_mean, grad_cov, axes, lengths): axes [D, D] holds the principal axes of cov as unit ROWS and lengths [D] their
        standard deviations (square roots of cov's eigenvalues), largest first.  ValueError unless H is negative definite
        (x is no peak of the mean); a Matern-3/2 model is refused as mean_hessian refuses it."""
        x = np.asarray(self.xstar if x is None else x, dtype=float).reshape(-1)
        H = self.mean_hessian(x)
        top = float(np.linalg.eigvalsh(H).max())
        if not top < 0.0:
            raise ValueError(f"xstar_covariance: the mean Hessian at x is not negative definite (largest eigenvalue {top:.3e}): "
                             "x is no peak of the posterior mean")
        m, Cg = self.gradient_pred(x)
        m, Cg = m[0], Cg[0]
        cov = np.linalg.solve(H, np.linalg.solve(H, Cg).T)
        cov = 0.5 * (cov + cov.T)
        w, V = np.linalg.eigh(cov)
        order = np.argsort(w)[::-1]
        return dict(cov=cov, hessian=H, grad_mean=m, grad_cov=Cg, axes=V[:, order].T.copy(),
                    lengths=np.sqrt(np.maximum(w[order], 0.0)))

    def loosest_direction(self, x=None):
        """The direction in which the optimum is located worst -- the first principal axis of xstar_covariance(x) -- as a
        query direction, normalised |xi| / max |xi| the way next_query normalises its own."""
        xi = self.xstar_covariance(x)["axes"][0]
        return np.abs(xi) / np.max(np.abs(xi))

    def active_subspace(self, n_points=1024, seed=None, X=None):
        """(eigenvalues [D], eigenvectors [D, D] as unit ROWS), largest first, of E_x[grad f grad f'] = mean_i(m_i m_i' +
        C_i) over n_points uniform points of the unit box from np.random.default_rng(seed), or over the given points X: the
        directions along which the utility varies over the whole box, rotated ones included (effect_importance and
        sensitivity see coordinates only)."""
        post = self._var_post()
        if X is None:
            X = np.random.default_rng(seed).random((int(n_points), 6 if post.camphor is not None else post.X.shape[1]))
        X = X if isinstance(X, torch.Tensor) else np.atleast_2d(np.asarray(X, dtype=float))
        out = self.eng.predict_gradients(post, X, want_best=False)
        m, Cg = out["mean"], out["cov"]
        A = ((m.unsqueeze(2) * m.unsqueeze(1) + Cg).mean(dim=0)).cpu().numpy()
        A = 0.5 * (A + A.T)
        w, V = np.linalg.eigh(A)
        order = np.argsort(w)[::-1]
        return w[order], V[:, order].T.copy()

    def _choice_draws(self, n_draws, G, noisy, seed):
        """(z, e, noise_sd) of answer_pred / choice_pred: one ppbo_randn stream of 2 S G normals per seed, the first S G
        of them z, the next S G the likelihood's noise e (drawn whether or not it is used, so that the paths of a seed
        are the same with and without noise)."""
        S = int(n_draws)
        if S < 1:
            raise ValueError(f"n_draws = {n_draws}: at least one draw is required")
        if seed is None:
            from .random_fourier_sampler import draw_seed
            seed = draw_seed()
        ze = self.eng.randn(seed, 2, S, G)
        return ze[0], (ze[1] if noisy else None), (None if noisy else 0.0)

    def answer_pred(self, xi, x, alphas=None, n_draws=4096, noisy=True, seed=None):
        """Where on the query line {alpha xi + x} will the user stop?  (alphas [G], prob [G]) as NumPy arrays for one
        line, prob [B, G] for stacked xi, x [B, D]: the probability that the point at alphas[g] is the one marked, under
        the model's own likelihood (sum_Phi, gp_model.py:176-204: the marked point beats every other point of the line
        under utilities with noise theta[0]) -- the share of n_draws posterior draws of f on the line, plus that noise,
        whose maximum it is (ppbo_line_choice_xi; no reference counterpart).  alphas: the G <= 128 abscissae, by default
        the 70 equispaced points of EI's grid without its noise; noisy = False: the noise-free argmax of the posterior
        path.  (xi, x) in the scaled coordinates next_query(unscale=False) returns.  seed: None takes one off the global
        NumPy stream; a fixed seed gives bitwise-equal results."""
        post = self._var_post()
        xi, x = np.asarray(xi, dtype=float), np.asarray(x, dtype=float)
        if xi.shape != x.shape or xi.ndim not in (1, 2) or xi.shape[-1] != self.D or xi.shape[0] < 1:
            raise ValueError(f"answer_pred: xi and x of shapes {xi.shape} and {x.shape}; two [{self.D}] vectors or two "
                             f"[B, {self.D}] stacks are required")
        alphas = np.linspace(0.005, 0.995, 70) if alphas is None else np.asarray(alphas, dtype=float)
        if alphas.ndim != 1 or not 1 <= alphas.size <= 128:
            raise ValueError(f"answer_pred: alphas of shape {alphas.shape}; 1 .. 128 abscissae in a vector are required")
        z, e, noise_sd = self._choice_draws(n_draws, alphas.size, noisy, seed)
        out = self.eng.line_choice_xi(post, np.atleast_2d(xi), np.atleast_2d(x), alphas, z, e, noise_sd,
                                      self.COVARIANCE_SHRINKAGE, jitter=1e-10 * float(self.theta[2]) ** 2)
        prob = out["prob"].cpu().numpy()
        return alphas, (prob[0] if xi.ndim == 1 else prob)

    def choice_pred(self, X_items, n_draws=4096, noisy=True, seed=None):
        """Which of K shortlisted configurations will the user pick?  X_items [K, D] -> prob [K], or [B, K, D] ->
        [B, K] for B shortlists (K <= 128), as NumPy: the probability that each item is the one picked, by the model
        and the draws of answer_pred (ppbo_line_choice on arbitrary points).  K = 2 is preference_pred's p up to
        Monte-Carlo error."""
        post = self._var_post()
        X = np.asarray(X_items, dtype=float)
        if X.ndim not in (2, 3) or X.shape[-1] != self.D or not 1 <= X.shape[-2] <= 128 or X.shape[0] < 1:
            raise ValueError(f"choice_pred: items of shape {X.shape}; [K, {self.D}] or [B, K, {self.D}] with 1 <= K <= 128 "
                             "is required")
        z, e, noise_sd = self._choice_draws(n_draws, X.shape[-2], noisy, seed)
        out = self.eng.line_choice(post, X if X.ndim == 3 else X[None], z, e, noise_sd, self.COVARIANCE_SHRINKAGE,
                                   jitter=1e-10 * float(self.theta[2]) ** 2)
        prob = out["prob"].cpu().numpy()
        return prob[0] if X.ndim == 2 else prob

    # ------------------------------------------------------------------ scoring the answers
    def _loo(self, P, f, theta, n_draws, seed):
        """Engine.loo_answers on a posterior covariance P and mode f (device), with answer_pred's jitter and seed rule."""
        S = int(n_draws)
        if S < 1:
            raise ValueError(f"n_draws = {n_draws}: at least one draw is required")
        if seed is None:
            from .random_fourier_sampler import draw_seed
            seed = draw_seed()
        return self.eng.loo_answers(P, f, self.m, float(theta[0]), S=S, seed=seed, jitter=1e-10 * float(theta[2]) ** 2)

    def loo_pred(self, n_draws=4096, seed=None):
        """How well does the model explain each answer it was trained on?  Leave-one-query-out in its cavity form
        (ppbo_loo_answers; no reference counterpart): query q's likelihood site is taken out of the Laplace posterior --
        no refit -- and the remaining belief is asked how probable the answer was.  A dict of NumPy arrays: lpd [n_q] the
        log predictive score (n_draws Monte-Carlo draws of the star likelihood), agreement [n_q] the mean probability that
        the chosen point beats another point of its line, edge_prob [n_q, m] those probabilities, cav_mean and cav_var
        [N] the cavity's mean and variance at the design rows, info [n_q] (0 fine; 1 / 2: the block of P / the cavity is not
        positive definite and the query's scores are NaN).  It reads only the posterior covariance and f_MAP, whatever the
        kernel.  seed: None takes one off the global NumPy stream; a fixed seed gives bitwise-equal results."""
        post = self._var_post()
        if post.P is None:           # as posterior_covariance: formed on demand
            self._post = post = self.eng.posterior(self._dX, self.theta, self.kernel.__name__, self._dSigma_inv,
                                                   self.eng.dev(self.fMAP), self.m, want_P=True)
        out = self._loo(post.P, self.eng.dev(self.fMAP), self.theta, n_draws, seed)
        edge = out["edge"].cpu().numpy()
        return dict(lpd=out["lpd"].cpu().numpy(), agreement=out["agreement"].cpu().numpy(), edge_prob=edge[:, 1:],
                    cav_mean=out["cav_mean"].cpu().numpy(), cav_var=out["cav_var"].cpu().numpy(),
                    info=out["info"].cpu().numpy())

    def inconsistent_answers(self, k=5, n_draws=4096, seed=None):
        """The k answers the model explains worst -- candidates for a slip of the slider: dict(query [k] the queries with
        the lowest leave-one-out log score, lowest first, lpd [k], agreement [k], X [k, m + 1, D] their rows of the design,
        the chosen point first)."""
        r = self.loo_pred(n_draws, seed)
        lpd = np.where(np.isnan(r["lpd"]), -np.inf, r["lpd"])          # a query that could not be scored comes first
        order = np.argsort(lpd, kind="stable")[:max(int(k), 0)]
        b = self.m + 1
        return dict(query=order, lpd=r["lpd"][order], agreement=r["agreement"][order],
                    X=np.asarray(self.X).reshape(-1, b, self.D)[order])

    def answers_score(self, X_stars, n_draws=4096, seed=None):
        """The held-out score of new answers under the full posterior (ppbo_score_answers; no reference counterpart), the
        test-set number for comparing kernels and hyper-parameters.  X_stars [n (m + 1), D]: n stars in
        FeedbackProcessing's row layout (the chosen point, then its m pseudo-observations), in the coordinates of the
        design.  dict(lpd [n], agreement [n], edge_prob [n, m], total = sum lpd)."""
        post = self._var_post()
        X = np.asarray(X_stars, dtype=float)
        b = self.m + 1
        if X.ndim != 2 or X.shape[1] != self.D or X.shape[0] < b or X.shape[0] % b or not 2 <= b <= 128:
            raise ValueError(f"answers_score: stars of shape {X.shape}; [n ({b}), {self.D}] with n >= 1 and at most 128 rows "
                             "per star is required")
        S = int(n_draws)
        if S < 1:
            raise ValueError(f"n_draws = {n_draws}: at least one draw is required")
        if seed is None:
            from .random_fourier_sampler import draw_seed
            seed = draw_seed()
        out = self.eng.score_answers(post, X.reshape(-1, b, self.D), S=S, seed=seed, shrink=self.COVARIANCE_SHRINKAGE,
                                     jitter=1e-10 * float(self.theta[2]) ** 2)
        lpd = out["lpd"].cpu().numpy()
        return dict(lpd=lpd, agreement=out["agreement"].cpu().numpy(), edge_prob=out["edge"].cpu().numpy()[:, 1:],
                    total=float(lpd.sum()))

    def loo_score(self, theta=None, n_draws=4096, seed=None):
        """sum_q lpd_q, the leave-one-query-out log score of the design: of the fitted model (theta = None: the sum of
        loo_pred's lpd for the same seed), or of a fit at `theta` by the evidence's route (Gram matrix, inverse, f_MAP from
        the current one, posterior), which leaves the model's own state alone.  NaN where a query cannot be scored."""
        if theta is None:
            return float(self.loo_pred(n_draws, seed)["lpd"].sum())
        theta = _theta_list(theta)
        f0 = self.eng.dev(self.fMAP) if getattr(self, "fMAP", None) is not None else self.eng.dev(np.zeros(self.N))
        _, Sinv, fm, _, _, _ = self._evidence_fit(self.eng, theta, f0.reshape(-1).clone())
        post = self.eng.posterior(self._dX, theta, self.kernel.__name__, Sinv, fm, self.m, want_P=True)
        return float(self._loo(post.P, fm, theta, n_draws, seed)["lpd"].sum().item())

    @staticmethod
    def _numpy(out):
        return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}

    def tournament_pred(self, XA, XB):
        """Every candidate XA[i] against every opponent XB[j] (ppbo_predict_tournament; no reference counterpart), as a
        dict of NumPy arrays: mu_a, var_a [Ma], mu_b, var_b [Mb], cov [Ma, Mb] = cov(f(a_i), f(b_j)), prob [Ma, Mb] =
        P(a_i > b_j), score [Ma] = the Borda score (mean of row i of prob), best_val / best_idx its maximum and first
        row.  At most 1024 opponents per call; for near-ties (a ~ b) preference_pred keeps more digits of var_d."""
        post = self._var_post()
        return self._numpy(self.eng.predict_tournament(post, np.atleast_2d(np.asarray(XA, dtype=float)),
                                                       np.atleast_2d(np.asarray(XB, dtype=float)), want_cov=True,
                                                       want_prob=True))

    def default_field(self, n_field=256, seed=None):
        """The default field of borda_pred: n_field uniform points of the unit box from np.random.default_rng(seed)."""
        return np.random.default_rng(seed).random((int(n_field), self.D))

    def borda_pred(self, X, field=None, n_field=256, seed=None):
        """(score [M], winner): the Borda (soft-Copeland) score of each row of X -- its probability of beating an
        opponent drawn at random from `field` [Mb, D] (default: default_field(n_field, seed)) -- and the index of the
        row with the largest score.  No M x Mb matrix is formed."""
        post = self._var_post()
        field = self.default_field(n_field, seed) if field is None else np.atleast_2d(np.asarray(field, dtype=float))
        out = self.eng.predict_tournament(post, np.atleast_2d(np.asarray(X, dtype=float)), field)
        return out["score"].cpu().numpy(), int(out["best_idx"])

    def ranking_pred(self, X_items):
        """(P [K, K], borda [K], order [K]) for K <= 1024 shortlisted configurations: the win matrix P[i, j] =
        P(item i > item j) (diagonal 1/2 to ~1e-8), each item's Borda score against the shortlist and the items ordered
        from the highest score down (stable: of equal scores the lower index first).  The companion of choice_pred."""
        post = self._var_post()
        X = np.asarray(X_items, dtype=float)
        if X.ndim != 2 or X.shape[1] != self.D or not 1 <= X.shape[0] <= 1024:
            raise ValueError(f"ranking_pred: items of shape {X.shape}; [K, {self.D}] with 1 <= K <= 1024 is required")
        out = self.eng.predict_tournament(post, X, X, want_prob=True, want_best=False)
        borda = out["score"].cpu().numpy()
        return out["prob"].cpu().numpy(), borda, np.argsort(-borda, kind="stable")

    def shortlist(self, q=8, score="EI", X_cand=None, noise_var=None):
        """(X [q, D], idx [q], score [q]): the q configurations worth showing next, picked greedily by `score` -- "EI"
        (pointwise expected improvement over self.mustar) or "variance" -- under the posterior variance conditioned on
        the earlier picks (ppbo_search_batch; no reference counterpart), so the picks spread over the basins instead of
        crowding the best one.  The producer of the item sets that choice_pred, ranking_pred and tournament_pred
        consume.  X_cand [M, D]: the candidates in the caller's coordinates; by default the resident candidate pool
        under a fresh rotation, and idx then indexes those rotated rows.  noise_var: the noise of the imagined
        observations (None: theta[0]^2; 0: exact).  X comes back in the caller's coordinates; picks that found nothing
        scoreable left (fewer than q candidates, non-finite rows) are dropped."""
        kinds = {"EI": SCORE_POINTWISE_EI, "variance": SCORE_VARIANCE}
        if score not in kinds:
            raise ValueError(f"shortlist: score {score!r}; \"EI\" or \"variance\" is required")
        post = self._var_post()
        if X_cand is None:
            cand = self.eng.shift_points(self._candidate_pool(), np.random.uniform(0.0, 1.0, self.D))
        elif isinstance(X_cand, torch.Tensor):
            cand = self.eng.dev(X_cand if X_cand.dim() == 2 else X_cand.reshape(1, -1))
        else:
            cand = self.eng.dev(np.atleast_2d(np.asarray(X_cand, dtype=float)))
        out = self.eng.search_batch(post, cand, int(q), score=kinds[score],
                                    mustar=0.0 if self.mustar is None else float(self.mustar), noise_var=noise_var)
        keep = out["idx"] >= 0
        idx = out["idx"][keep]
        X = cand[torch.as_tensor(idx, device=cand.device)].cpu().numpy() if idx.size else np.zeros((0, self.D))
        return X, idx, out["score"][keep]

    def kg_field(self, n=64):
        """[<= n, D]: the field of knowledge_gradient -- the points whose means compete for the maximum after the imagined
        observation: xstar first, then the local maxima xstars_local, then shortlist(q, "EI") picks for the rows that are
        left.  The current recommendation xstar MUST be in the field: h(0), the maximum of the mean now, is taken over
        the field and the candidate, so a field without it understates the present answer and inflates every KG."""
        n = int(n)
        if not 1 <= n <= 1024:
            raise ValueError(f"kg_field: n = {n}; 1 .. 1024 is required")
        if self.xstar is None:
            raise RuntimeError("kg_field: no recommendation yet (xstar is None): update the model first")
        rows = [np.asarray(self.xstar, dtype=float).reshape(1, self.D)]
        if self.xstars_local is not None and len(self.xstars_local):
            rows.append(np.asarray(self.xstars_local, dtype=float).reshape(-1, self.D))
        field = np.concatenate(rows)[:n]
        while len(field) < n:                    # (a shortlist holds at most 64 picks)
            q = min(n - len(field), 64)
            picks = self.shortlist(q=q, score="EI")[0]
            field = np.concatenate([field, picks])
            if len(picks) < q:
                break
        return field

    def knowledge_gradient(self, X_cand=None, field=None, noise_var=None):
        """dict(kg [M], best_idx, x [D], field [Mb, D], mu [M], var [M]): the knowledge gradient for correlated beliefs
        (Frazier, Powell and Dayanik 2009; ppbo_predict_kg, no reference counterpart) of every candidate -- the expected
        rise of the maximum of the posterior mean over `field` and the candidate itself after one observation AT the
        candidate -- with the row of the largest one (best_idx, x) and the candidates' mean and variance.  Pointwise EI
        and the variance score a candidate by its own marginal; this scores it by what it does to argmax mu, the answer
        users take from the model.
        The imagined observation is the shortlist's convention, "f(x) observed with Gaussian noise noise_var" (None:
        theta[0]^2; 0: exact).  It is NOT the answer to a preference query: a PPBO query returns a choice among the
        points of a line, not a noisy value of f, so KG ranks where knowing f would help most, not queries.
        X_cand [M, D]: the candidates in the caller's coordinates; by default the resident candidate pool under a fresh
        rotation, as in shortlist, and best_idx then indexes those rotated rows.  field [Mb <= 1024, D]: by default
        kg_field(); a field of one's own should hold xstar (see kg_field)."""
        post = self._var_post()
        field = self.kg_field() if field is None else np.atleast_2d(np.asarray(field, dtype=float))
        if X_cand is None:
            cand = self.eng.shift_points(self._candidate_pool(), np.random.uniform(0.0, 1.0, self.D))
        elif isinstance(X_cand, torch.Tensor):
            cand = self.eng.dev(X_cand if X_cand.dim() == 2 else X_cand.reshape(1, -1))
        else:
            cand = self.eng.dev(np.atleast_2d(np.asarray(X_cand, dtype=float)))
        out = self.eng.predict_kg(post, cand, field, noise_var=noise_var)
        b = int(out["best_idx"])
        return dict(kg=out["kg"].cpu().numpy(), best_idx=b, x=cand[b].cpu().numpy() if b >= 0 else None, field=field,
                    mu=out["mu_a"].cpu().numpy(), var=out["var_a"].cpu().numpy())

    _ACQ_KINDS = {"mean": SCORE_MEAN, "EI": SCORE_POINTWISE_EI, "variance": SCORE_VARIANCE}

    def acquisition_grad(self, X, score="EI"):
        """dict(mu, var, score [M], grad_mu, grad_var, grad_score [M, D]) as NumPy arrays: the posterior mean, the variance
        and the acquisition `score` -- "EI" (pointwise expected improvement over self.mustar), "variance" or "mean" -- at
        the rows of X with their analytic gradients, in the caller's coordinates (ppbo_acq_grad; no reference
        counterpart).  One point may be given as a 1-D vector."""
        if score not in self._ACQ_KINDS:
            raise ValueError(f"acquisition_grad: score {score!r}; \"EI\", \"variance\" or \"mean\" is required")
        post = self._var_post()
        X = X if isinstance(X, torch.Tensor) else np.asarray(X, dtype=float)
        X = X.reshape(1, -1) if X.ndim == 1 else X
        return self._numpy(self.eng.acq_grad(post, X, score=self._ACQ_KINDS[score],
                                             mustar=0.0 if self.mustar is None else float(self.mustar)))

    def maximize_acquisition(self, score="EI", n_starts=16, X_cand=None, lower=None, upper=None, fixed=None, iters=60):
        """The continuous maximiser of the acquisition `score` ("EI" or "variance") inside the box lower <= x <= upper with
        the coordinates of `fixed` ({d: value}) held: shortlist(q=n_starts, score, X_cand)'s picks -- spread over the
        basins by the conditioned variance -- clipped into the box, each refined by the device ascent on the analytic
        gradient (ppbo_acq_ascent; no reference counterpart), then the best.  Returns dict(x [D], score, mu, var, starts
        [K, D], start_scores [K] (the shortlist's, at the time of each pick), xs [K, D], scores [K], iters [K]).  The
        ascent is monotone, so with the default box scores[k] is never below the score of starts[k]."""
        kinds = {"EI": SCORE_POINTWISE_EI, "variance": SCORE_VARIANCE}
        if score not in kinds:
            raise ValueError(f"maximize_acquisition: score {score!r}; \"EI\" or \"variance\" is required")
        lo, hi = self._box(lower, upper, fixed)
        post = self._var_post()
        starts, _, start_scores = self.shortlist(q=int(n_starts), score=score, X_cand=X_cand)
        if not len(starts):
            raise ValueError("maximize_acquisition: the shortlist found no scoreable candidate")
        out = self._numpy(self.eng.acq_ascent(post, starts, score=kinds[score],
                                              mustar=0.0 if self.mustar is None else float(self.mustar), lower=lo, upper=hi,
                                              iters=int(iters)))
        ok = np.flatnonzero(~np.isnan(out["score"]))
        if not ok.size:
            raise ValueError("maximize_acquisition: no start has a score")
        b = int(ok[np.argmax(out["score"][ok])])
        return dict(x=out["x"][b].copy(), score=float(out["score"][b]), mu=float(out["mu"][b]), var=float(out["var"][b]),
                    starts=starts, start_scores=start_scores, xs=out["x"], scores=out["score"], iters=out["iters"])

    def mu_pred(self, X_pred):
        x = np.asarray(X_pred, dtype=float).reshape(1, self.D)
        out = self.eng.predict(self._mean_post(), x, score=SCORE_MEAN, want_var=False, want_best=False)
        return float(out["mu"].item())

    def mu_pred_neq(self, X_pred):
        return -self.mu_pred(X_pred)

    def mu_pred_batch(self, X_pred):
        """Posterior mean of many points in one launch (device tensor in, NumPy out)."""
        out = self.eng.predict(self._mean_post(), X_pred, score=SCORE_MEAN, want_var=False, want_best=False)
        return out["mu"].cpu().numpy()

    # ------------------------------------------------------------------ maximiser of the posterior mean
    def _ascend(self, starts):
        """Projected gradient ascent on the posterior mean from K starts at once (ppbo_mean_ascent: Barzilai-Borwein
        step lengths, monotone safeguard, the whole iteration of a start inside one workgroup).  SURVEY 8(f) f-2."""
        xs, mus, _ = self.eng.mean_ascent(self._mean_post(), np.clip(np.atleast_2d(starts).astype(float), 0.0, 1.0),
                                          iters=ASCENT_ITERS, tol=1e-9)
        return xs.cpu().numpy(), mus.cpu().numpy()

    def _polish(self, x0):
        """Bounded quasi-Newton polish of one point with the analytic device gradient."""
        post = self._mean_post()

        def fg(x):
            mu, g = self.eng.mean_grad(post, np.clip(x, 0.0, 1.0)[None, :])
            return -float(mu.cpu().numpy()[0]), -g.cpu().numpy()[0]

        res = scipy.optimize.minimize(fg, x0, jac=True, method="L-BFGS-B", bounds=self.bounds,
                                      options={"maxiter": 200, "ftol": 1e-15, "gtol": 1e-10})
        return np.clip(res.x, 0.0, 1.0), -float(res.fun)

    def _candidate_pool(self):
        """SEARCH_CANDIDATES uniform points, drawn ONCE from the global NumPy stream and kept resident in HBM; every
        mu_star trial sees them through a fresh random rotation frac(pool + shift) (ppbo_shift_points), which
        keeps them uniform -- instead of generating and uploading 65536 x D numbers per trial."""
        pool = self.__dict__.get("_pool")
        if pool is None or pool.shape[1] != self.D:
            pool = self.eng.dev(np.random.uniform(0.0, 1.0, (SEARCH_CANDIDATES, self.D)))
            self._pool = pool
        return pool

    def mu_star(self, mustar_finding_trials=None):
        """argmax of the posterior mean (gp_model.py:415-437).  The reference runs SciPy differential evolution
        `trials` times (2 k ... 17 k sequential mu_pred calls each); here a trial is ONE device enqueue
        (ppbo_mean_search): score 65536 rotated pool candidates plus the design points and the previous x*, keep the
        ASCENT_STARTS best that are > 0.05 apart, run the whole Barzilai-Borwein ascent of each inside one kernel;
        the host reads ASCENT_STARTS x (D + 1) numbers back and polishes the winner.  All distinct converged maxima
        feed xstars_local (gp_model.py:430-431)."""
        import torch
        trials = self.mustar_finding_trials if mustar_finding_trials is None else mustar_finding_trials
        D, N = self.D, self.N
        post = self._mean_post()
        pool = self._candidate_pool()
        # ALL trials in one enqueue (ppbo_mean_search_multi): each sees the resident pool through its own rotation, formed
        # on the fly; one screening launch, one thinning launch, one start-selection launch (a workgroup per trial), one
        # ascent launch of trials x ASCENT_STARTS workgroups.  (Rounds 3-4 ran one ppbo_mean_search per trial on three
        # stream / ctx lanes: 3 trials at C3 2.0-2.3 ms, their kernels mostly serialised.)
        # The design points (where f_MAP's maxima sit) and the previous x* join the first trial only: they would claim
        # the same ASCENT_STARTS basins in every trial and leave the uniform candidates' basins unexplored.
        shifts = np.stack([np.random.uniform(0.0, 1.0, D) for _ in range(trials)]) if trials > 0 else np.zeros((0, D))
        xprev = np.asarray(self.xstar if self.xstar is not None else self.X[0], dtype=float).reshape(D)
        queued = []
        for t0 in range(0, trials, 64):                                # the entry takes up to 64 trials
            xs_d, mu_d = self.eng.mean_search_multi(post, pool, shifts[t0:t0 + 64], "design" if t0 == 0 else None,
                                                    xprev if t0 == 0 else None, K=ASCENT_STARTS, sep=5e-2,
                                                    iters=ASCENT_ITERS, tol=1e-9, screen_fp32=self.mustar_screen_fp32)
            queued.append((xs_d, mu_d))
        found, winners, winner_mu = [], [], {}
        if queued:
            all_x = torch.cat([q[0] for q in queued]).cpu().numpy()              # [trials, K, D]
            all_v = torch.cat([q[1] for q in queued]).cpu().numpy()              # [trials, K], -inf = no start
            per_trial = []
            for t in range(trials):
                ok = np.isfinite(all_v[t])
                xs, vals = all_x[t][ok], all_v[t][ok]
                per_trial.append((xs, vals))
                if len(vals):
                    winners.append((t, int(np.argmax(vals))))
            if winners:
                # the ascent stops on |projected gradient| * step < 1e-9; the quasi-Newton polish (a device round
                # trip per function value) is only worth its milliseconds when a winner is NOT yet stationary
                wx = np.stack([per_trial[t][0][b] for t, b in winners])
                mw, gw = self.eng.mean_grad(post, wx)
                mg = torch.cat([mw.reshape(-1, 1), gw], dim=1).cpu().numpy()       # one read-back: mu | grad per winner
                def stationary(x, gb, v):
                    pg = np.where(((x <= 0.0) & (gb < 0.0)) | ((x >= 1.0) & (gb > 0.0)), 0.0, gb)
                    return np.abs(pg).max() <= POLISH_GRAD_TOL * max(abs(v), 1e-300)
                todo = []
                for k, ((t, b), row) in enumerate(zip(winners, mg)):
                    xs, vals = per_trial[t]
                    if stationary(xs[b], row[1:], vals[b]):
                        # mu_pred at this point, already on the host (the same K*' alpha in fp64 by mean_grad_kernel): if it
                        # ends up as x*, mustar needs no further device round trip
                        winner_mu[xs[b].tobytes()] = float(row[0])
                    else:
                        todo.append((t, b))
                if todo:
                    # winners the 100-evaluation ascent left short of stationarity: ONE more device ascent for all of them
                    # (four times the budget, a tighter step tolerance) before anything goes through SciPy -- the
                    # quasi-Newton polish costs a device round trip per function value
                    self.polish_log["device_reascents"] += len(todo)
                    p0 = np.stack([per_trial[t][0][b] for t, b in todo])
                    xa, ma, _ = self.eng.mean_ascent(post, p0, iters=4 * ASCENT_ITERS, tol=1e-12)
                    ma2, ga = self.eng.mean_grad(post, xa)
                    xa, rows = xa.cpu().numpy(), torch.cat([ma2.reshape(-1, 1), ga], dim=1).cpu().numpy()
                    for (t, b), xk, row in zip(todo, xa, rows):
                        xs, vals = per_trial[t]
                        if row[0] >= vals[b]:
                            xs[b], vals[b] = xk, float(row[0])
                        if stationary(xs[b], row[1:], vals[b]) and row[0] >= vals[b]:
                            winner_mu[xs[b].tobytes()] = float(row[0])
                            continue
                        self.polish_log["scipy_polishes"] += 1
                        xp, vp = self._polish(xs[b])
                        if vp >= vals[b]:
                            xs[b], vals[b] = xp, vp
            for xs, vals in per_trial:
                found.extend(zip(vals.tolist(), xs))
        if not found:                 # no finite mean anywhere (cannot happen with a fitted model): keep the old x*
            x0 = self.xstar if self.xstar is not None else self.X[0]
            return np.asarray(x0, dtype=float).reshape(D,), self.mu_pred(x0), np.asarray(x0, dtype=float).reshape(1, D)
        found.sort(key=lambda p: -p[0])
        xstar = found[0][1].copy()
        # distinct maxima > 0.1 apart, best first (gp_model.py:430-431): one distance matrix, then a greedy sweep that
        # strikes everything within 0.1 of a kept maximum (the pairwise Python loop this replaces cost 10 ms at D = 20,
        # where 3 trials return ~90 converged points and ~45 distinct maxima: more than the searches themselves)
        P = np.stack([x for _, x in found])
        sq = (P * P).sum(axis=1)
        d2 = np.maximum(sq[:, None] + sq[None, :] - 2.0 * (P @ P.T), 0.0)
        struck = np.zeros(len(P), dtype=bool)
        keep = []
        for i in range(len(P)):
            if not struck[i]:
                keep.append(i)
                struck |= d2[i] <= 1e-2
        xstars_local = P[keep].reshape(-1, D)
        mustar = winner_mu.get(xstar.tobytes())
        return xstar.reshape(D,), (self.mu_pred(xstar) if mustar is None else mustar), xstars_local

    # ------------------------------------------------------------------ maximisers inside boxes
    def _box(self, lower=None, upper=None, fixed=None):
        """(lo [D], hi [D]) in the model's unit coordinates from bounds and a dict {d: value} of fixed coordinates."""
        D = int(self.D)
        lo = np.zeros(D) if lower is None else np.array(lower, dtype=float).reshape(-1)
        hi = np.ones(D) if upper is None else np.array(upper, dtype=float).reshape(-1)
        if lo.size != D or hi.size != D:
            raise ValueError(f"bounds of {lo.size} and {hi.size} entries for a model of {D} dimensions")
        for d, v in (fixed or {}).items():
            if not 0 <= int(d) < D:
                raise ValueError(f"fixed coordinate {d} of a model of {D} dimensions")
            lo[int(d)] = hi[int(d)] = float(v)
        if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all((0.0 <= lo) & (lo <= hi) & (hi <= 1.0))):
            raise ValueError("a box needs 0 <= lower <= upper <= 1 in every coordinate")
        return lo, hi

    def mu_star_in(self, lower=None, upper=None, fixed=None, trials=None):
        """(x, mu, xstars_local): the maximiser of the posterior mean inside the box lower <= x <= upper with the
        coordinates of `fixed` ({d: value}) held -- a conditional optimum, a trust region, or both; bounds in the model's
        unit coordinates, like X.  mu_star's recipe inside the box, every trial in one enqueue (ppbo_mean_search_boxes):
        the resident pool rotated per trial and mapped into the box, the current x* clipped into it as a seed,
        ASCENT_STARTS ascents per trial more than 0.05 of the longest side apart, and one more device ascent inside the box
        (four times the budget) for a trial's winner that is not yet stationary.  xstars_local: the distinct maxima found
        (more than 0.1 of the longest side apart), best first."""
        lo, hi = self._box(lower, upper, fixed)
        D = int(self.D)
        trials = max(1, int(self.mustar_finding_trials if trials is None else trials))
        post = self._mean_post()
        side = float((hi - lo).max())
        box = np.stack([lo, hi])
        shifts = np.stack([np.random.uniform(0.0, 1.0, D) for _ in range(trials)])
        seed = np.asarray(self.xstar if self.xstar is not None else self.X[0], dtype=float).reshape(1, 1, D)
        xs_d, mu_d, _ = self.eng.mean_search_boxes(post, self._candidate_pool(), np.tile(box, (trials, 1, 1)), shifts=shifts,
                                                   seeds=np.tile(seed, (trials, 1, 1)), K=ASCENT_STARTS, sep=5e-2 * side,
                                                   iters=ASCENT_ITERS, tol=1e-9, screen_fp32=self.mustar_screen_fp32)
        all_x, all_v = xs_d.cpu().numpy(), mu_d.cpu().numpy()
        best = np.argmax(all_v, axis=1)                                  # found rows come first, -inf behind them
        wx, wv = all_x[np.arange(trials), best], all_v[np.arange(trials), best]
        _, gw = self.eng.mean_grad(post, wx)
        gw = gw.cpu().numpy()
        pg = np.where(((wx <= lo) & (gw < 0.0)) | ((wx >= hi) & (gw > 0.0)), 0.0, gw)
        todo = np.flatnonzero(np.abs(pg).max(axis=1) > POLISH_GRAD_TOL * np.maximum(np.abs(wv), 1e-300))
        if todo.size:
            self.polish_log["device_reascents"] += int(todo.size)
            xa, ma, _ = self.eng.mean_ascent_boxes(post, wx[todo], box[None], per_box=int(todo.size), iters=4 * ASCENT_ITERS,
                                                   tol=1e-12)
            xa, ma = xa.cpu().numpy(), ma.cpu().numpy()
            for j, t in enumerate(todo):
                if ma[j] >= all_v[t, best[t]]:
                    all_x[t, best[t]], all_v[t, best[t]] = xa[j], ma[j]
        ok = np.isfinite(all_v)
        P, v = all_x[ok], all_v[ok]
        order = np.argsort(-v, kind="stable")
        P, v = P[order], v[order]
        sq = (P * P).sum(axis=1)
        d2 = np.maximum(sq[:, None] + sq[None, :] - 2.0 * (P @ P.T), 0.0)
        struck, keep = np.zeros(len(P), dtype=bool), []
        for i in range(len(P)):
            if not struck[i]:
                keep.append(i)
                struck |= d2[i] <= (0.1 * side) ** 2
                struck[i] = True
        return P[0].copy(), float(v[0]), P[keep].reshape(-1, D)

    def conditional_xstar(self, fixed):
        """(x, mu, xstars_local): the best configuration with the coordinates of `fixed` ({d: value}) held at their
        values and the others free -- mu_star_in with nothing but `fixed`."""
        return self.mu_star_in(fixed=fixed)

    def _profile(self, dims, values):
        """max over the other coordinates of the posterior mean with x[dims] = values[t] for each row t of values [T, n]:
        ONE ppbo_mean_search_boxes call of T boxes.  Trial t is seeded with x* and every known local maximum moved onto
        its slice (x[dims] := values[t]), so the profile never falls below the slice through x*.  Returns mu [T], x [T, D],
        var [T]."""
        D = int(self.D)
        T = values.shape[0]
        if T * PROFILE_STARTS > 65536 or T > 4096:
            raise ValueError(f"a profile of {T} grid points: at most {min(4096, 65536 // PROFILE_STARTS)} in one call")
        if not np.all((values >= 0.0) & (values <= 1.0)):
            raise ValueError("grid values outside the unit interval")
        post = self._mean_post()
        boxes = np.tile(np.stack([np.zeros(D), np.ones(D)]), (T, 1, 1))
        boxes[:, :, dims] = values[:, None, :]
        x0 = np.asarray(self.xstar if self.xstar is not None else self.X[0], dtype=float).reshape(1, D)
        pts = x0 if self.xstars_local is None else np.vstack([x0, np.asarray(self.xstars_local, dtype=float).reshape(-1, D)])
        seeds = np.tile(pts[:64][None], (T, 1, 1))
        seeds[:, :, dims] = values[:, None, :]
        pool = self._candidate_pool()[:PROFILE_CANDIDATES]
        xs_d, mu_d, _ = self.eng.mean_search_boxes(post, pool, boxes, shifts=None, seeds=seeds, K=PROFILE_STARTS, sep=5e-2,
                                                   iters=ASCENT_ITERS, tol=1e-9, screen_fp32=self.mustar_screen_fp32)
        xs, mus = xs_d.cpu().numpy(), mu_d.cpu().numpy()
        best = np.argmax(mus, axis=1)
        x, mu = xs[np.arange(T), best], mus[np.arange(T), best]
        var = self.eng.predict(self._var_post(), x, want_mu=False, want_var=True, want_best=False)["var"].cpu().numpy()
        return mu, x, var

    def profile_effect(self, d, grid=None):
        """The profile of coordinate d (0-based): for every t of the grid the largest posterior mean over all points with
        x_d = t, max over the OTHER coordinates -- how good the utility can still get as a function of x_d.  It
        complements main_effect, which averages the others out (and needs a product kernel): a profile exists for every
        kernel family, and unlike a slice through x* it does not understate the utility where coordinates interact.
        Returns a dict t [T], mu [T], x [T, D] (the maximisers, x[:, d] == t), var [T] (the posterior variance there).
        Default grid: 65 equispaced points of [0, 1]."""
        g = self._effect_grid(grid)
        if not 0 <= int(d) < int(self.D):
            raise ValueError(f"coordinate {d} of a model of {self.D} dimensions")
        mu, x, var = self._profile([int(d)], g.reshape(-1, 1))
        return dict(t=g, mu=mu, x=x, var=var)

    def profile_interaction(self, d, e, grid_d=None, grid_e=None):
        """The two-dimensional profile over grid_d x grid_e (default 33 equispaced points each): mu [Td, Te] the largest
        posterior mean with x_d and x_e held, x [Td, Te, D] its maximisers, var [Td, Te]; one search call for the whole
        grid.  Returns a dict t_d, t_e, mu, x, var."""
        gd, ge = self._effect_grid(grid_d, 33), self._effect_grid(grid_e, 33)
        D = int(self.D)
        if not (0 <= int(d) < D and 0 <= int(e) < D and int(d) != int(e)):
            raise ValueError(f"coordinates {d}, {e} of a model of {D} dimensions: two different ones are required")
        t = np.stack(np.meshgrid(gd, ge, indexing="ij"), axis=-1).reshape(-1, 2)
        mu, x, var = self._profile([int(d), int(e)], t)
        return dict(t_d=gd, t_e=ge, mu=mu.reshape(gd.size, ge.size), x=x.reshape(gd.size, ge.size, D),
                    var=var.reshape(gd.size, ge.size))
