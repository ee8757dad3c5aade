"""Drop-in Hsampler (src/random_fourier_sampler.py): random-Fourier-feature posterior samples of
the utility and their maximisers, with the feature projection, the weight-space Laplace terms
and the candidate scoring evaluated by the HIP kernels (ppbo_rff_project / _terms / _score).

Differences in *cost*, not in results: the reference's weight-space Hessian is diagonal
(:118-122) but is returned, inverted and sampled as a dense F x F matrix (:134-140, 207-213);
here the diagonal is kept as a vector (the dense forms are still produced on request for
attribute compatibility).  The L-BFGS-B multi-start of return_xstar (:143-176) is one device
enqueue: batched candidate scoring, start selection and the whole multi-start gradient ascent (ppbo_rff_search).

Spectral bases (the reference has the SE one only, :40-42): SE, RQ (alpha = 2, a Gamma scale mixture of SE), the
Matern kernels (Student-t) and the camphor-copper kernels.  camphor(x, x'; l_0..l_5) = SE(e(x), e(x'); 1) for the
11-column embedding e of engine.py / include/ppbo_hip.h, so a camphor basis is the unit SE basis on e: W is [F, 11],
Phi(X) is formed on the embedded rows, and every method that takes or returns a point works in the caller's six
coordinates (phi / Dphi through e and its Jacobian; the search by ppbo_rff_search_camphor).

Beyond the reference: sample_paths draws from the GP's own Laplace posterior by Matheron's rule (PosteriorPaths:
g_s = phi^T w_s + k(., X) v_s, ppbo_path_score_multi / ppbo_path_search_multi), where the weight-space posterior above keeps
only a diagonal covariance; sample_xstars(..., posterior="pathwise") searches those paths.
"""
from __future__ import annotations

import time

import numpy as np

from .engine import RFF_MULTI_MAX_S, camphor_lengthscales, get_engine

SCORE_CANDIDATES = 65536
RFF_STARTS = 32            # refined starts per posterior sample (the reference: 5-30 L-BFGS-B runs)


# smoothness nu of the Matern kernels (kernels.py); their spectral density is a multivariate Student-t
MATERN_NU = {"Matern52_kernel": 2.5, "Matern32_kernel": 1.5}


def matern_spectral_draw(F, D, lengthscale, nu, rng=np.random):
    """F frequencies [F, D] from the spectral density of Matern(nu) with length scale l: a multivariate Student-t with
    2 nu degrees of freedom and scale I / l^2, drawn as W = z / l * sqrt(2 nu / u), z ~ N(0, I_D), u ~ chi^2_{2 nu} per
    feature.  E|w|^2 = D (2 nu / (2 nu - 2)) / l^2."""
    z = rng.standard_normal((F, D))
    u = rng.chisquare(2.0 * nu, size=F)
    return z / lengthscale * np.sqrt(2.0 * nu / u)[:, None]


RQ_ALPHA = 2.0               # the reference's RQ kernel fixes alpha = 2 (src/kernels.py:27-34)
CAMPHOR_KERNELS = ("camphor_copper_kernel", "camphor_copper_ard_kernel")
CAMPHOR_E = 11               # width of the camphor embedding e(x)


def rq_spectral_draw(F, D, lengthscale, alpha=RQ_ALPHA, rng=np.random):
    """F frequencies [F, D] from the spectral density of RQ(alpha) with length scale l.  (1 + r^2 / (2 alpha l^2))^-alpha
    = E_tau[exp(-tau r^2 / (2 l^2))] with tau ~ Gamma(shape alpha, rate alpha), so a draw is the SE draw of length scale
    l / sqrt(tau): W = z sqrt(tau) / l, z ~ N(0, I_D), one tau per feature.  Draw order: the F x D normals, then the F
    gammas."""
    z = rng.standard_normal((F, D))
    tau = rng.gamma(alpha, 1.0 / alpha, size=F)
    return z * np.sqrt(tau)[:, None] / lengthscale


def camphor_embed_host(x, ls):
    """e(x) [n, 11] of caller rows x [n, 6]: (cos 2 pi x_d, sin 2 pi x_d) / l_d for d != 2, x_2 / l_2 for z, in the
    column order (c0, s0, c1, s1, z, c3, s3, c4, s4, c5, s5) of include/ppbo_hip.h."""
    x = np.atleast_2d(np.asarray(x, dtype=float))
    cols = []
    for d in range(6):
        if d == 2:
            cols.append(x[:, 2] / ls[2])
        else:
            cols += [np.cos(2 * np.pi * x[:, d]) / ls[d], np.sin(2 * np.pi * x[:, d]) / ls[d]]
    return np.stack(cols, axis=1)


def camphor_embed_jacobian(x, ls):
    """de/dx [11, 6] at one caller point x: d c_d / d x_d = -2 pi s_d, d s_d / d x_d = 2 pi c_d, d z / d x_2 = 1 / l_2."""
    e = camphor_embed_host(x, ls)[0]
    J = np.zeros((CAMPHOR_E, 6))
    c = 0
    for d in range(6):
        if d == 2:
            J[c, 2] = 1.0 / ls[2]
            c += 1
        else:
            J[c, d] = -2 * np.pi * e[c + 1]
            J[c + 1, d] = 2 * np.pi * e[c]
            c += 2
    return J


def draw_seed(rng=np.random):
    """A 63-bit seed for the device draws from the global NumPy stream (np.random.seed keeps whole runs reproducible)."""
    return int(rng.randint(0, 2 ** 62)) * 2 + int(rng.randint(0, 2))


def omega_draws_host(omega_map, cov_diag, z):
    """The batched weight draw Omega[s] = omega_MAP + sqrt(cov_diag) z[s] (ppbo_rff_omega_draws) for given normals z."""
    return np.asarray(omega_map, dtype=float) + np.sqrt(np.asarray(cov_diag, dtype=float)) * np.asarray(z, dtype=float)


def best_per_sample(x, val, found):
    """Per sample s of a batched search (x [S, K, D], val [S, K], found [S]): the best of its refined maxima (rows
    < found[s], finite values only) -> (X [S, D], V [S], the samples without one).  Those rows of X / V hold NaN."""
    x, val, found = np.asarray(x, dtype=float), np.asarray(val, dtype=float), np.asarray(found).ravel()
    S, K = val.shape
    live = (np.arange(K)[None, :] < found[:, None]) & np.isfinite(val)
    v = np.where(live, val, -np.inf)
    k = np.argmax(v, axis=1)
    ok = live.any(axis=1)
    X = np.where(ok[:, None], x[np.arange(S), k], np.nan)
    V = np.where(ok, v[np.arange(S), k], np.nan)
    return X, V, np.flatnonzero(~ok)


class PosteriorPaths:
    """n pathwise (decoupled, Wilson et al. 2020) samples of the utility from the GP's Laplace posterior,

        g_s(x) = phi(x)^T w_s + k(x, X) v_s,     w_s ~ N(0, I_F),   v_s = Sigma^-1 (f_s - Phi(X)^T w_s),   f_s ~ N(f_MAP, P)

    W_prior [n, F] and V [n, N] stay on the device; the basis, design, kernel and theta are the sampler's at the time of
    the draw (made by Hsampler.sample_paths)."""

    def __init__(self, sampler, W_prior, V):
        self._hs = sampler
        self.eng = sampler.eng
        self.W_prior, self.V = W_prior, V
        self.n = int(W_prior.shape[0])
        self.kernel, self.theta = sampler.kernel, sampler.theta
        self._W, self._b, self._X = sampler._dev("W"), sampler._dev("b"), sampler._dev("X")

    def evaluate(self, Xq):
        """g_s(x_q) for every path: a [n, M] device tensor (ppbo_path_score_multi, RFF_MULTI_MAX_S paths per launch)."""
        import torch
        Xq = self.eng.dev(Xq)
        out = [self.eng.path_score_multi(Xq, self._W, self._b, self.theta, self.kernel, self._X, self.W_prior[c0:c0 + RFF_MULTI_MAX_S],
                                         self.V[c0:c0 + RFF_MULTI_MAX_S]) for c0 in range(0, self.n, RFF_MULTI_MAX_S)]
        return out[0] if len(out) == 1 else torch.cat(out, dim=0)

    def xstars(self, starts=RFF_STARTS):
        """(X [n, D], values [n]): the best refined maximiser of every path over the candidates of return_xstar and
        g_s there (ppbo_path_search_multi).  A path whose search finds nothing is a RuntimeError."""
        work = self._hs._xstar_candidates()
        X, V = np.empty((self.n, work.shape[1])), np.empty(self.n)
        for c0 in range(0, self.n, RFF_MULTI_MAX_S):
            c1 = min(self.n, c0 + RFF_MULTI_MAX_S)
            X[c0:c1], V[c0:c1], missing = best_per_sample(*self.eng.path_search_multi(
                work, self._W, self._b, self.theta, self.kernel, self._X, self.W_prior[c0:c1], self.V[c0:c1], K=starts, iters=100))
            if missing.size:
                raise RuntimeError(f"PosteriorPaths.xstars: {missing.size} paths found no maximiser")
        return X, V


class Hsampler:
    def __init__(self, gp_model, nFeatures=1000, engine=None):
        self.eng = engine if engine is not None else getattr(gp_model, "eng", None) or get_engine()
        self.nFeatures = nFeatures
        self.b = None
        self.W = None
        self.D = gp_model.D
        self.m = gp_model.m
        self.X = gp_model.X
        self.GP_xstar = gp_model.xstar
        self.GP_xstars_local = gp_model.xstars_local
        self.n_gausshermite_sample_points = gp_model.n_gausshermite_sample_points
        self.obs_indices = gp_model.obs_indices
        self.kernel = str(gp_model.kernel.__name__)
        self.theta = gp_model.theta
        self._phi_X = None        # host copy of Phi(X), made on first access (67 MB at C3: 5 ms nobody needs per update)
        self.omega_MAP = None
        self.cov_diag = None      # the posterior covariance of omega is diagonal (S_hessian is): this is its diagonal
        self._hess_diag = None
        self.verbose = False
        self._dPhi = None
        # the model's resident uniform candidate pool (GPModel._candidate_pool: drawn once per model, rotated per use),
        # shared instead of drawing and uploading 65536 x D fresh uniforms per sampler (4 ms of a 13 ms cycle at D = 20)
        self._pool_of = getattr(gp_model, "_candidate_pool", None)
        # device copies of W, b and X, made once per ARRAY OBJECT (assigning a new array refreshes them; the basis is 655 KB
        # at F = 4096, D = 20, and every projection / search used to upload it again)
        self._dcache = {}
        dX = getattr(gp_model, "_dX", None)
        if dX is not None and tuple(dX.shape) == tuple(np.shape(self.X)) and dX.device == self.eng.device:
            self._dcache["X"] = (self.X, dX)
        # camphor kernels: the six length scales, and the model's posteriors whose embedded rows e(X) can be reused
        self.camphor_l = camphor_lengthscales(self.theta, self.D) if self.kernel in CAMPHOR_KERNELS else None
        self._posts = (getattr(gp_model, "_post", None), getattr(gp_model, "_post_mean", None))
        self._gp = gp_model       # sample_paths reads the fit (Sigma_inv, fMAP, posterior_covariance) when it is called

    def _dev(self, name):
        arr = getattr(self, name)
        hit = self._dcache.get(name)
        if hit is None or hit[0] is not arr:
            hit = (arr, self.eng.dev(np.asarray(arr, dtype=float).ravel() if name == "b" else arr))
            self._dcache[name] = hit
        return hit[1]

    # ---- basis -----------------------------------------------------------------
    def generate_basis(self):
        # per-dimension length scales (ARD): column d of W is divided by l_d -- the spectral density of the scaled kernel --
        # with the same draws in the same order as a scalar l
        if self.kernel in CAMPHOR_KERNELS:
            # the unit SE basis on the embedding: the length scales live in e(x)
            self.camphor_l = camphor_lengthscales(self.theta, self.D)
            self.W = np.random.randn(self.nFeatures, CAMPHOR_E)
        else:
            ls = self.theta[1] if np.ndim(self.theta[1]) == 0 else np.asarray(self.theta[1], dtype=float)
            if self.kernel == "SE_kernel":                        # the reference supports the SE spectral density only (:40-42)
                self.W = np.random.randn(self.nFeatures, self.D) / ls
            elif self.kernel in MATERN_NU:
                self.W = matern_spectral_draw(self.nFeatures, self.D, ls, MATERN_NU[self.kernel])
            elif self.kernel == "RQ_kernel":
                self.W = rq_spectral_draw(self.nFeatures, self.D, ls)
            else:
                raise ValueError(f"Hsampler has no spectral basis for the kernel {self.kernel!r}")
        self.b = np.random.uniform(low=0, high=2 * np.pi, size=self.nFeatures)[:, None]

    # ---- camphor: the embedding --------------------------------------------------
    def _camphor(self):
        """The six camphor length scales, or None for the other kernels."""
        if self.kernel not in CAMPHOR_KERNELS:
            return None
        l = self.__dict__.get("camphor_l")
        if l is None:
            l = self.camphor_l = camphor_lengthscales(self.theta, self.D)
        return l

    def _check_W(self):
        """A basis whose width does not fit the kernel (11 for camphor, D otherwise) would be read as another basis."""
        want = CAMPHOR_E if self._camphor() is not None else self.D
        if np.ndim(self.W) != 2 or np.shape(self.W)[1] != want:
            raise ValueError(f"Hsampler.W has shape {np.shape(self.W)}: [nFeatures, {want}] required for {self.kernel}")

    def _dev_embedded_X(self):
        """Device copy of e(X) [N, 11]: the posterior's own embedded rows where the model has them at these length
        scales, else ppbo_camphor_embed of X; made once per X object."""
        l = self._camphor()
        hit = self._dcache.get("E")
        if hit is not None and hit[0] is self.X and np.array_equal(hit[1], l):
            return hit[2]
        E = None
        for post in self.__dict__.get("_posts", ()):
            if (post is not None and post.camphor is not None and np.array_equal(post.camphor, l)
                    and tuple(post.X.shape) == (np.shape(self.X)[0], CAMPHOR_E)):
                E = post.X
                break
        if E is None:
            E = self.eng.camphor_embed(self._dev("X"), l)
        self._dcache["E"] = (self.X, l.copy(), E)
        return E

    def _points(self, Xc):
        """Caller-coordinate points -> the rows the basis acts on (embedded for camphor, else as they are)."""
        l = self._camphor()
        return Xc if l is None else self.eng.camphor_embed(Xc, l)

    def _scale(self):
        return np.sqrt(2.0 * self.theta[2] ** 2 / self.nFeatures)

    def phiVec(self, x):
        self._check_W()
        x = np.atleast_2d(np.asarray(x, dtype=float))
        return self.eng.rff_project(self._points(x), self.W, self.b.ravel(), self.theta[2]).cpu().numpy()

    def phi(self, x):
        self._check_W()
        l = self._camphor()
        x = np.asarray(x, dtype=float)
        e = x if l is None else camphor_embed_host(x, l)[0]
        return self._scale() * np.cos(self.W @ e + self.b.ravel())

    def Dphi(self, x):
        self._check_W()
        l = self._camphor()
        x = np.asarray(x, dtype=float)
        if l is None:
            return -self._scale() * np.sin(self.W @ x + self.b.ravel())[:, None] * self.W
        e = camphor_embed_host(x, l)[0]
        return -self._scale() * np.sin(self.W @ e + self.b.ravel())[:, None] * (self.W @ camphor_embed_jacobian(x, l))

    def DDphi(self, x):
        raise NotImplementedError

    def update_phi_X(self):
        self._check_W()
        X = self._dev("X") if self._camphor() is None else self._dev_embedded_X()
        self._dPhi = self.eng.rff_project(X, self._dev("W"), self._dev("b"), self.theta[2])
        self._phi_X = None

    @property
    def phi_X(self):
        """Phi(X) [F, N] as a NumPy array (random_fourier_sampler.py:57-58); lives on the device, copied on demand."""
        if self._phi_X is None and self._dPhi is not None:
            self._phi_X = self._dPhi.cpu().numpy()
        return self._phi_X

    @phi_X.setter
    def phi_X(self, value):
        self._phi_X = None if value is None else np.asarray(value, dtype=float)
        self._dPhi = None if value is None else self.eng.dev(self._phi_X)

    @property
    def covariance_inv(self):
        """-S_hessian(omega_MAP) as the dense F x F matrix the reference stores (:136); built on demand."""
        return None if self._hess_diag is None else np.diag(self._hess_diag)

    @property
    def covariance(self):
        """The dense F x F posterior covariance of the reference (:137); built on demand from its diagonal."""
        return None if self.cov_diag is None else np.diag(self.cov_diag)

    # ---- weight-space Laplace terms ------------------------------------------------
    def _terms(self, omega, theta):
        return self.eng.rff_terms(self._dPhi, omega, self.m, theta[0])

    def S(self, omega, theta):
        return self._terms(omega, theta)[0]

    def S_grad(self, omega, theta):
        return self._terms(omega, theta)[1].cpu().numpy()

    def S_hessian_diag(self, omega, theta):
        return self._terms(omega, theta)[2].cpu().numpy()

    def S_hessian(self, omega, theta):
        return np.diag(self.S_hessian_diag(omega, theta))

    # ---- the reference's per-query helpers of S (random_fourier_sampler.py:62-102), kept for callers that use them;
    # S / S_grad / S_hessian above do NOT go through them (ppbo_rff_terms sums over all queries in one pass)
    def sum_Phi(self, i, order_of_derivative, f, sigma, sample_points=None, weights=None):
        """Query i (an element of obs_indices): order 0 -> sum_j Phi(Delta_j / sqrt 2) (scalar, closed form of the
        Gauss-Hermite integral); order 1 -> sum_j (phi_X[:, i+1+j] - phi_X[:, i]) var2_normal_pdf(Delta_j) (a vector
        of nFeatures); order 2 -> sum_j -(phi_X[:, i+1+j] - phi_X[:, i])^2 Delta_j / 2 var2_normal_pdf(Delta_j).  The
        per-pseudo-observation weights come from ppbo_sum_phi's kernel family (ppbo_laplace_terms), the feature
        contractions from the device GEMM on the resident Phi(X)."""
        if order_of_derivative not in (0, 1, 2):
            print("The derivatives of an order higher than 2 are not needed!")
            return None
        i, m = int(i), self.m
        f = np.asarray(f, dtype=float).ravel()
        if order_of_derivative == 0:
            return float(self.eng.sum_phi(f, m, sigma, 0).cpu().numpy()[i // (m + 1)])
        # beta (order 1) and Lambda's off-diagonal (order 2) carry exactly these weights, up to their scale factors
        _, beta, _, lo = self.eng.laplace_terms(f, m, sigma)
        blk = slice(i + 1, i + m + 1)
        if order_of_derivative == 1:
            w = -(beta[blk] * (sigma * m))                    # var2_normal_pdf(Delta_j)
        else:
            w = lo[blk] * (m * sigma ** 2)                    # -Delta_j / 2 var2_normal_pdf(Delta_j)
        diff = self._dPhi[:, blk] - self._dPhi[:, i:i + 1]    # [F, m] on the device
        if order_of_derivative == 2:
            diff = diff * diff
        return self.eng.dgemm(diff.contiguous(), w.reshape(-1, 1).contiguous()).cpu().numpy().ravel()

    def sum_Phi_vec(self, order_of_derivative, f, sigma):
        """One sum_Phi per observation (random_fourier_sampler.py:96-102): [n_q] for order 0, [n_q, nFeatures] else."""
        out = [self.sum_Phi(i, order_of_derivative, f, sigma) for i in self.obs_indices]
        return None if any(o is None for o in out) else np.array(out)

    def update_omega_MAP(self):
        """Maximise S from a standard-normal start (:124-132).  The Hessian is diagonal, so the
        trust-region Newton of the reference reduces to per-coordinate safeguarded Newton steps."""
        omega = np.random.randn(self.nFeatures)
        start = time.time()
        # the whole trust-region loop runs behind one call (ppbo_rff_omega_map) and on the device: omega, gradient,
        # Hessian diagonal and the region's state stay there, S / |grad S| / the iteration count come back once
        omega, S, gnorm, iters = self.eng.rff_omega_map(self._dPhi, omega, self.m, self.theta[0], maxiter=500, gtol=1e-6)
        self.omega_MAP_stats = {"S": S, "gradnorm": gnorm, "iterations": iters}
        if self.verbose:
            print("... this took " + str(time.time() - start) + " seconds.")
        self.omega_MAP = omega

    def update_covariancematrix(self):
        hd = -self.S_hessian_diag(self.omega_MAP, self.theta)
        if np.any(hd <= 0):
            print("---!!!--- Posterior covariance matrix is not PSD ---!!!---")
            return
        self._hess_diag = hd
        self.cov_diag = 1.0 / hd

    def sample_omega(self):
        if self.cov_diag is None:
            print("Omega sampler error! Omega MAP-estimate was used instead.")
            return self.omega_MAP
        return self.omega_MAP + np.sqrt(self.cov_diag) * np.random.standard_normal(self.nFeatures)

    # ---- maximiser of one posterior sample --------------------------------------------
    def score_candidates(self, Xc, omega):
        """phi(x)^T omega for many candidates on the device; returns (scores, best value, best index)."""
        self._check_W()
        sc, bv, bi = self.eng.rff_score(self._points(Xc), self._dev("W"), self._dev("b"), self.theta[2], omega)
        return sc.cpu().numpy(), bv, bi

    def return_xstar(self, omega):
        """argmax_x phi(x)^T omega (:143-176).  The reference runs 5-30 L-BFGS-B searches from perturbed local maxima
        of the posterior mean on NumPy phi / Dphi; here ONE device enqueue (ppbo_rff_search) scores a rotated resident
        uniform pool plus such perturbations, keeps the RFF_STARTS best that are > 0.05 apart and runs the whole
        projected gradient ascent of each inside one kernel; the best refined point is returned."""
        self._check_W()
        start = time.time()
        work = self._xstar_candidates()
        # 100 Barzilai-Borwein iterations per start: the winning start is stationary after ~50 (tests/probes/
        # rff_ascent_scale.py: the same maximum at 50, 100 and 200), the cap only bounds the starts that keep bouncing
        l = self._camphor()
        if l is None:
            xs, vals = self.eng.rff_search(work, self._dev("W"), self._dev("b"), self.theta[2], omega, K=RFF_STARTS, iters=100)
        else:       # camphor: the same pool and starts in the caller's coordinates, features on the embedding
            xs, vals = self.eng.rff_search_camphor(work, l, self._dev("W"), self._dev("b"), self.theta[2], omega,
                                                   K=RFF_STARTS, iters=100)
        if self.verbose:
            print("Optimization of f_approx took " + str(time.time() - start) + " seconds.")
        if len(vals) == 0 or not np.isfinite(vals).any():
            return None
        return xs[int(np.nanargmax(vals))]

    def _xstar_candidates(self):
        """The candidates of a maximiser search: the model's resident uniform pool under a fresh rotation, followed by
        uniform perturbations of GP_xstars_local (a [M + k, D] device tensor; draws from the global NumPy stream)."""
        import torch
        D = self.D
        pool = self.__dict__.get("_pool")
        if pool is None:
            shared = self._pool_of() if self._pool_of is not None else None
            if shared is not None and shared.shape[1] == D and shared.device == self.eng.device:
                pool = self._pool = shared
            else:
                pool = self._pool = self.eng.dev(np.random.uniform(0, 1, (SCORE_CANDIDATES, D)))
        M = pool.shape[0]
        loc = np.atleast_2d(self.GP_xstars_local)
        k = min(len(loc) * 64, SCORE_CANDIDATES // 4)
        near = np.clip(loc[np.random.randint(len(loc), size=k)] + 0.01 * np.random.uniform(0, 1, (k, D)), 0, 1)
        work = torch.empty((M + k, D), dtype=torch.float64, device=self.eng.device)
        self.eng.shift_points(pool, np.random.uniform(0, 1, D), out=work[:M])
        work[M:].copy_(self.eng.dev(near))
        return work

    def return_xstar_for_dim(self, omega, dim, x_ref):
        self._check_W()
        x_ref = np.array(x_ref, dtype=float)
        grid = np.tile(x_ref, (4096, 1))
        grid[:, dim - 1] = np.linspace(0, 1, 4096)
        _, _, bi = self.eng.rff_score(self._points(grid), self._dev("W"), self._dev("b"), self.theta[2], omega,
                                      want_score=False)
        return grid[bi]

    def sample_xstar(self):
        xstar = None
        while xstar is None:
            xstar = self.return_xstar(self.sample_omega())
        return xstar

    # ---- the posterior distribution of the maximiser: many samples per call ----------------------
    def sample_omegas(self, n, seed=None):
        """[n, nFeatures] draws of the weights from N(omega_MAP, diag(cov_diag)) on the device (ppbo_rff_omega_draws),
        bitwise reproducible for a seed; seed=None takes one from the global NumPy stream.  Unlike sample_omega there
        is no fallback to omega_MAP: without a covariance it raises RuntimeError."""
        if self.cov_diag is None or self.omega_MAP is None:
            raise RuntimeError("Hsampler.sample_omegas: no posterior covariance (run update_omega_MAP and "
                               "update_covariancematrix first)")
        if seed is None:
            seed = draw_seed()
        return self.eng.rff_omega_draws(seed, self._dev("omega_MAP"), self._dev("cov_diag"), int(n))

    def sample_paths(self, n, seed=None):
        """n pathwise samples of the utility from the GP's Laplace posterior (PosteriorPaths): prior weights W_prior
        [n, F] and normals z [n, N] from the ppbo_randn stream of `seed` (W_prior[s, f] at index s F + f, z[s, i] at
        n F + s N + i: bitwise reproducible; seed=None takes one from the global NumPy stream), f_s = f_MAP + L z_s with
        L L^T = posterior_covariance (ppbo_potrf), V = (F_s - W_prior Phi(X)) Sigma^-1 (three ppbo_dgemm on the resident
        Phi(X) and Sigma^-1).  The fit is read from the gp_model the sampler was built on; without one it raises
        RuntimeError.  Not for the camphor-copper kernels."""
        import torch
        if self._camphor() is not None:
            raise NotImplementedError(f"Hsampler.sample_paths: pathwise samples are not implemented for {self.kernel}")
        self._check_W()
        n = int(n)
        if n < 1:
            raise ValueError(f"sample_paths: n = {n} samples")
        gp = self.__dict__.get("_gp")
        Sinv = getattr(gp, "_dSigma_inv", None)
        if Sinv is None:
            Sinv = getattr(gp, "Sigma_inv", None)
        fmap = getattr(gp, "fMAP", None)
        P = getattr(gp, "posterior_covariance", None) if (Sinv is not None and fmap is not None) else None
        if P is None:
            raise RuntimeError("Hsampler.sample_paths: no fitted posterior (run update_model on the GP model first)")
        post = getattr(gp, "_post", None)
        if getattr(post, "P", None) is not None:
            P = post.P                                         # the device copy behind the NumPy attribute
        N = np.shape(self.X)[0]
        if tuple(Sinv.shape) != (N, N) or tuple(P.shape) != (N, N) or np.size(fmap) != N:
            raise RuntimeError(f"Hsampler.sample_paths: the GP model's fit is not of this sampler's design ({N} points): "
                               "run update_model, then build the sampler")
        if self._dPhi is None or tuple(self._dPhi.shape) != (np.shape(self.W)[0], N):
            raise RuntimeError("Hsampler.sample_paths: no Phi(X) of this basis (run update_phi_X first)")
        F = self._dPhi.shape[0]
        if seed is None:
            seed = draw_seed()
        eng = self.eng
        draws = eng.randn(seed, n * (F + N))
        W_prior, z = draws[:n * F].view(n, F), draws[n * F:].view(n, N)
        L = torch.tril(eng.potrf_(eng.dev(P).clone()))
        Fs = eng.dev(fmap).reshape(1, N).repeat(n, 1)
        eng.dgemm(z, L, transB=True, beta=1.0, C_out=Fs)                  # F_s = f_MAP + z L^T
        eng.dgemm(W_prior, self._dPhi, alpha=-1.0, beta=1.0, C_out=Fs)    # ... - W_prior Phi(X)
        V = eng.dgemm(Fs, eng.dev(Sinv))                                  # Sigma^-1 is symmetric
        return PosteriorPaths(self, W_prior, V)

    def sample_xstars(self, n, omegas=None, seed=None, starts=RFF_STARTS, posterior="weights"):
        """n samples of the maximiser x* of the posterior utility: (X [n, D], values [n]), row k the best refined
        maximiser of sample k in the caller's coordinates (camphor: [n, 6]) and phi(x)^T omega_k there.  What n calls
        of sample_xstar compute, in batches of up to RFF_MULTI_MAX_S samples per device enqueue (ppbo_rff_search_multi):
        the candidates are built once per call as in return_xstar and shared by all samples.  omegas [n, F] (host or
        device) replaces the device draws.  A sample whose search finds nothing is redrawn once per batch; if its
        redraw finds nothing either, RuntimeError.
        posterior="pathwise": the samples are paths of the GP's own Laplace posterior instead,
        sample_paths(n, seed).xstars(starts) (omegas does not apply); any other value is a ValueError."""
        if posterior not in ("weights", "pathwise"):
            raise ValueError(f"sample_xstars: posterior = {posterior!r} ('weights' or 'pathwise')")
        if posterior == "pathwise":
            if omegas is not None:
                raise ValueError("sample_xstars: omegas are draws of the weight-space posterior, not of posterior='pathwise'")
            return self.sample_paths(n, seed).xstars(starts)
        self._check_W()
        n = int(n)
        if n < 1:
            raise ValueError(f"sample_xstars: n = {n} samples")
        F = self.nFeatures if self.W is None else np.shape(self.W)[0]
        if omegas is None:
            omegas = self.sample_omegas(n, seed)
        elif tuple(omegas.shape) != (n, F):
            raise ValueError(f"sample_xstars: omegas of shape {tuple(omegas.shape)}, [{n}, {F}] required")
        omegas = self.eng.dev(omegas)
        work = self._xstar_candidates()
        l = self._camphor()

        def search(om):
            if l is None:
                return self.eng.rff_search_multi(work, self._dev("W"), self._dev("b"), self.theta[2], om, K=starts,
                                                 iters=100)
            return self.eng.rff_search_multi_camphor(work, l, self._dev("W"), self._dev("b"), self.theta[2], om,
                                                     K=starts, iters=100)

        X = np.empty((n, self.D if l is None else 6))
        V = np.empty(n)
        for c0 in range(0, n, RFF_MULTI_MAX_S):
            c1 = min(n, c0 + RFF_MULTI_MAX_S)
            X[c0:c1], V[c0:c1], missing = best_per_sample(*search(omegas[c0:c1]))
            if missing.size:
                # as sample_xstar: a sample without a maximiser is drawn again (once per batch, here)
                xr, vr, still = best_per_sample(*search(self.sample_omegas(missing.size)))
                if still.size:
                    raise RuntimeError(f"sample_xstars: {still.size} redrawn samples found no maximiser")
                X[c0 + missing], V[c0 + missing] = xr, vr
        return X, V

    def sample_xstar_for_dim(self, dim, x_ref):
        return self.return_xstar_for_dim(self.sample_omega(), dim, x_ref)
