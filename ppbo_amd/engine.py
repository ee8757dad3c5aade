"""Thin Python layer over the C-ABI: torch-ROCm tensors own the device buffers,
every computation is a call into libppbo_hip.so.  No NumPy math, no fallback."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import KERNEL_IDS, SCORE_MEAN, SCORE_POINTWISE_EI, SCORE_VARIANCE, PPBO_ERR_NOT_PD  # noqa: F401
from ._lib import PAIR_MEAN, PAIR_VARIANCE, PAIR_PROB  # noqa: F401
from ._lib import SLOPE_MEAN, SLOPE_VARIANCE, SLOPE_PROB  # noqa: F401
from ._lib import CURV_MEAN, CURV_VARIANCE, CURV_PROB  # noqa: F401
from ._lib import GRAD_NONE, GRAD_TRACE, GRAD_NORM2  # noqa: F401
from ._lib import FUNCTIONAL_MEAN, FUNCTIONAL_VARIANCE, FUNCTIONAL_PROB, FUNCTIONAL_MAX_G  # noqa: F401
from ._lib import EFFECT_RAW, EFFECT_CENTRED, EFFECT_INTERACTION, MARGINAL_MAX_DC  # noqa: F401
from ._lib import TOURNAMENT_BORDA, TOURNAMENT_WORST, TOURNAMENT_MAX_B  # noqa: F401
from ._lib import BATCH_MAX_Q, KG_MAX_B  # noqa: F401

# Posterior.form: which variance operator G holds (include/ppbo_hip.h, PPBO_FORM_*)
FORM_NODE = 0   # G = R Lambda, block lower triangular [N, N]
FORM_EDGE = 1   # H = L22^-1 of the edge-coordinate factor, rows / columns [n_q, N)

RFF_MULTI_MAX_S = 1024  # PPBO_RFF_MULTI_MAX_S: posterior samples per batched RFF enqueue (include/ppbo_hip.h)
SHRINKAGE = 1e-6  # COVARIANCE_SHRINKAGE of the reference (gp_model.py:26)

# ARD (one length scale per input dimension, no reference counterpart) is defined for these: for a radial kernel
# k(x, x'; l_1..l_D) = k(s (.) x, s (.) x'; l = 1) with s_d = 1 / l_d, so an ARD posterior stores its rows scaled once and
# every device path runs on them unchanged with theta = [sigma, 1, sigma_f]
RADIAL_KERNELS = ("SE_kernel", "RQ_kernel", "Matern52_kernel", "Matern32_kernel")

# camphor-copper with one length scale per coordinate (no reference counterpart): with e(x) in R^11 the embedding of
# include/ppbo_hip.h, camphor(x, x'; l_0..l_5) = SE(e(x), e(x'); 1), so such a posterior stores its rows embedded and the
# device sees SE with theta = [sigma, 1, sigma_f].  A scalar l is the reference's profile (l, l, l + 0.05, l, l, l).
CAMPHOR_ARD = "camphor_copper_ard_kernel"
CAMPHOR_PROFILE = np.array([0.0, 0.0, 0.05, 0.0, 0.0, 0.0])
# the kernels whose length scales the evidence gradient and optimize_theta_ard fit one by one
ARD_KERNELS = RADIAL_KERNELS + (CAMPHOR_ARD,)


def camphor_lengthscales(theta, D):
    """The six length scales of camphor_copper_ard_kernel: theta[1] a length-6 vector, or a scalar l standing for the
    profile (l, l, l + 0.05, l, l, l).  Raises ValueError unless D == 6 and every entry is positive and finite."""
    if D != 6:
        raise ValueError(f"{CAMPHOR_ARD} needs D == 6, not {D}")
    l = theta[1]
    v = float(l) + CAMPHOR_PROFILE if np.ndim(l) == 0 else np.asarray(l, dtype=np.float64).copy()
    if v.ndim != 1 or v.size != 6:
        raise ValueError(f"theta[1] has shape {v.shape}: a scalar or one length scale per coordinate (6) is required")
    if not (np.all(np.isfinite(v)) and np.all(v > 0)):
        raise ValueError("theta[1]: every camphor length scale must be positive and finite")
    return v


def camphor_embed_directions(X, Xi, ls):
    """J_e(x_i) xi_i [M, 11] for caller rows X [M, 6] and directions Xi [M, 6]: the derivative of the embedding e of
    include/ppbo_hip.h (columns c0, s0, c1, s1, z, c3, s3, c4, s4, c5, s5) along xi, d c_d = -2 pi sin(2 pi x_d) xi_d / l_d,
    d s_d = 2 pi cos(2 pi x_d) xi_d / l_d, d z = xi_2 / l_2.  NumPy in and out."""
    X, Xi = np.asarray(X, dtype=np.float64), np.asarray(Xi, dtype=np.float64)
    ls = np.asarray(ls, dtype=np.float64)
    cols = []
    for d in range(6):
        if d == 2:
            cols.append(Xi[:, 2] / ls[2])
        else:
            w = 2.0 * np.pi * Xi[:, d] / ls[d]
            cols += [-np.sin(2.0 * np.pi * X[:, d]) * w, np.cos(2.0 * np.pi * X[:, d]) * w]
    return np.stack(cols, axis=1)


def camphor_embed_accelerations(X, Xi, ls):
    """d^2 e(x_i + a xi_i) / da^2 at a = 0 [M, 11], beside camphor_embed_directions: a straight line in the caller's six
    coordinates is a curved path in the embedding's eleven.  Each periodic pair (c_d, s_d) = (cos, sin)(2 pi x_d) / l_d is
    scaled by -(2 pi xi_d)^2; the z column is 0.  NumPy in and out."""
    X, Xi = np.asarray(X, dtype=np.float64), np.asarray(Xi, dtype=np.float64)
    ls = np.asarray(ls, dtype=np.float64)
    cols = []
    for d in range(6):
        if d == 2:
            cols.append(np.zeros(X.shape[0]))
        else:
            w = -(2.0 * np.pi * Xi[:, d]) ** 2 / ls[d]
            cols += [np.cos(2.0 * np.pi * X[:, d]) * w, np.sin(2.0 * np.pi * X[:, d]) * w]
    return np.stack(cols, axis=1)


def camphor_embed_jacobians(X, ls):
    """J_e(x_i) [M, 11, 6] for caller rows X [M, 6] as a torch tensor on X's device: the Jacobian of the embedding e whose
    action on a direction camphor_embed_directions forms (column order and formulas as there: row c_d holds
    -2 pi sin(2 pi x_d) / l_d, row s_d holds 2 pi cos(2 pi x_d) / l_d, row z holds 1 / l_2, each in column d)."""
    X = torch.as_tensor(X, dtype=torch.float64)
    ls = torch.as_tensor(np.asarray(ls, dtype=np.float64), device=X.device)
    J = torch.zeros(X.shape[0], 11, 6, dtype=torch.float64, device=X.device)
    row = 0
    for d in range(6):
        if d == 2:
            J[:, row, 2] = 1.0 / ls[2]
            row += 1
        else:
            w = 2.0 * np.pi / ls[d]
            J[:, row, d] = -torch.sin(2.0 * np.pi * X[:, d]) * w
            J[:, row + 1, d] = torch.cos(2.0 * np.pi * X[:, d]) * w
            row += 2
    return J


def camphor_pull_back(X, ls, mean, cov):
    """(J'm [M, 6], J'CJ [M, 6, 6]) for the gradient's mean [M, 11] and covariance [M, 11, 11] in the embedding's columns
    at the caller rows X [M, 6] (either may be None), as batched torch products; J'CJ is symmetrised, (A + A') / 2, so it
    is symmetric bit for bit.  A row of X with a non-finite coordinate comes out as NaN."""
    J = camphor_embed_jacobians(X, ls)
    Jt = J.transpose(1, 2)
    m6 = torch.bmm(Jt, mean.unsqueeze(2)).squeeze(2) if mean is not None else None
    c6 = None
    if cov is not None:
        c6 = torch.bmm(torch.bmm(Jt, cov), J)
        c6 = 0.5 * (c6 + c6.transpose(1, 2))
    return m6, c6


def lengthscales(theta, D, kernel):
    """The one check of theta[1]: None for a scalar length scale (today's path, left exactly as it is), else the
    length-D float64 vector of per-dimension length scales.  A vector is never collapsed to a scalar, even when its
    entries are equal.  Raises ValueError for a vector with the camphor-copper kernel, of the wrong length, or with an
    entry that is not positive and finite.  camphor_copper_ard_kernel: always the six length scales
    (camphor_lengthscales; a scalar is expanded to the reference's profile)."""
    if kernel == CAMPHOR_ARD:
        return camphor_lengthscales(theta, D)
    l = theta[1]
    if np.ndim(l) == 0:
        return None
    v = np.asarray(l, dtype=np.float64)
    if kernel not in RADIAL_KERNELS:
        raise ValueError(f"per-dimension length scales are defined for the radial kernels {RADIAL_KERNELS}, not {kernel}")
    if v.ndim != 1 or v.size != D:
        raise ValueError(f"theta[1] has shape {v.shape}: a scalar or one length scale per input dimension ({D}) is required")
    if not (np.all(np.isfinite(v)) and np.all(v > 0)):
        raise ValueError("theta[1]: every per-dimension length scale must be positive and finite")
    return v


def theta_key(theta):
    """theta as a hashable, comparable tuple (sigma, l, sigma_f), l a float or a tuple of floats (the caches that are
    keyed on theta)."""
    l = theta[1]
    return (float(theta[0]), float(l) if np.ndim(l) == 0 else tuple(float(v) for v in np.ravel(l)), float(theta[2]))


# ---- main effects and interactions (ppbo_predict_marginals): the host side of the axes and the rows of a call --------------
EFFECTS = {"raw": EFFECT_RAW, "centred": EFFECT_CENTRED, "interaction": EFFECT_INTERACTION}


def marginal_axis_params(kernel, theta, D, scale=None, camphor=None):
    """(l [Dc], periodic [Dc], I0 [Dc]) of the per-coordinate factors of a kernel that is a product over the caller's
    unit-box coordinates: SE with a scalar l or with per-dimension length scales (scale = 1 / l), the camphor-copper
    kernel with its profile (l, l, l + 0.05, l, l, l) or with six length scales (camphor).  I0 is the scaled Bessel value
    e^-a I0(a), a = 1 / l^2 (scipy.special.ive: never a product of two factors).  ValueError for any other kernel: RQ and
    the Matern kernels are radial, not products -- GPModel.average_pred samples the box instead."""
    from scipy.special import ive
    if camphor is not None or kernel == CAMPHOR_ARD:
        l = np.asarray(camphor if camphor is not None else camphor_lengthscales(theta, 6), dtype=float).reshape(-1)
        periodic = np.array([1, 1, 0, 1, 1, 1], dtype=np.intc)
    elif kernel == "camphor_copper_kernel":
        l = float(theta[1]) + CAMPHOR_PROFILE
        periodic = np.array([1, 1, 0, 1, 1, 1], dtype=np.intc)
    elif kernel == "SE_kernel":
        l = 1.0 / np.asarray(scale, dtype=float).reshape(-1) if scale is not None else np.full(int(D), float(theta[1]))
        periodic = np.zeros(l.size, dtype=np.intc)
    else:
        raise ValueError(f"predict_marginals: {kernel} is not a product over coordinates (SE_kernel, camphor_copper_kernel and "
                         f"{CAMPHOR_ARD} are); average_pred samples the box for a radial kernel")
    if l.size < 1 or l.size > MARGINAL_MAX_DC or not (np.all(np.isfinite(l)) and np.all(l > 0.0)):
        raise ValueError(f"predict_marginals: length scales {l} (1 .. {MARGINAL_MAX_DC} positive finite values)")
    return l, periodic, ive(0, 1.0 / (l * l))


def marginal_rows(dims, t, Dc, effect):
    """The rows of a predict_marginals call as (dims [M, 2] int32, t [M, 2] float64) in canonical form: axes ascending,
    -1 = unused and last, the value of an unused axis 0.  dims: [M, 2], [M, 1], or one-dimensional [M] = ONE axis per row
    (order 1, whatever M is: a single order-2 row is [[d, e]], never [d, e]); a scalar is one order-1 row; t has the
    shape of dims.  ValueError for an axis outside -1 .. Dc - 1, the same axis twice, a first axis of -1 with a second
    one, an interaction of order below 2, or shapes that do not fit."""
    dims = np.asarray(dims)
    if dims.size and not np.all(np.equal(np.mod(dims, 1), 0)):
        raise ValueError("predict_marginals: axes must be integers")
    dims = dims.astype(np.int64)
    t = np.asarray(t, dtype=float)
    if dims.ndim == 0 and t.ndim == 0:
        dims, t = dims.reshape(1, 1), t.reshape(1, 1)
    elif dims.ndim == 1 and t.ndim == 1 and dims.size == t.size:
        dims, t = dims.reshape(-1, 1), t.reshape(-1, 1)
    if dims.ndim != 2 or dims.shape[1] not in (1, 2) or t.shape != dims.shape or dims.shape[0] < 1:
        raise ValueError(f"predict_marginals: axes of shape {dims.shape} and values of shape {t.shape} ([M, 2] each)")
    if dims.shape[1] == 1:
        dims = np.concatenate([dims, np.full_like(dims, -1)], axis=1)
        t = np.concatenate([t, np.zeros_like(t)], axis=1)
    d, e = dims[:, 0], dims[:, 1]
    if np.any(dims < -1) or np.any(dims >= Dc):
        raise ValueError(f"predict_marginals: an axis outside -1 .. {Dc - 1}")
    if np.any((d == e) & (d >= 0)):
        raise ValueError("predict_marginals: a row names the same axis twice")
    if np.any((d < 0) & (e >= 0)):
        raise ValueError("predict_marginals: a first axis of -1 with a second one")
    if effect == EFFECT_INTERACTION and np.any(e < 0):
        raise ValueError("predict_marginals: an interaction needs two axes in every row")
    swap = (e >= 0) & (e < d)
    dims = np.where(swap[:, None], dims[:, ::-1], dims)
    t = np.where(swap[:, None], t[:, ::-1], t)
    t = np.where(dims < 0, 0.0, t)
    return np.ascontiguousarray(dims, dtype=np.int32), np.ascontiguousarray(t, dtype=np.float64)


class NotPositiveDefinite(RuntimeError):
    def __init__(self, msg, info=0):
        super().__init__(msg)
        self.info = info


@dataclass
class Posterior:
    """Device-resident posterior state consumed by predict / predict_cov / line_acq.  With per-dimension length scales
    (scale is not None) X holds the SCALED rows s (.) x_i and the device sees theta = [sigma, 1, sigma_f]; every Engine
    method that takes points takes them in the caller's coordinates and maps them."""
    kernel: str
    theta: tuple             # theta_key(theta): the caller's theta
    m: int
    X: torch.Tensor          # [N, D]
    alpha: torch.Tensor      # [N]   Sigma^-1 f_MAP
    lam_diag: torch.Tensor   # [N]   Lambda_MAP (star form)
    lam_off: torch.Tensor    # [N]
    G: torch.Tensor | None   # [N, N] the variance operator: R Lambda (form FORM_NODE) or H (FORM_EDGE)
    P: torch.Tensor | None = None  # posterior covariance (optional)
    Gt: torch.Tensor | None = None  # transpose of G in the one-launch scoring kernel's layout (formed on first use)
    scale: np.ndarray | None = None  # ARD: s_d = 1 / l_d (None: a scalar length scale)
    camphor: np.ndarray | None = None  # camphor_copper_ard_kernel: l_0..l_5; X then holds the embedded rows [N, 11]
    Xu: torch.Tensor | None = None     # ARD: the rows in the caller's unit-box coordinates (formed on first use, marginal_axes)
    Xc: torch.Tensor | None = None     # ... and this the caller's rows [N, 6] (mu_star searches in their coordinates)
    form: int = FORM_NODE              # FORM_NODE / FORM_EDGE: how G is to be read (ppbo_model.form)
    proj: object = None                # the cached VarianceProjection of G (Engine.project_variance); dropped with Gt

    @property
    def embedded(self):
        """The device works on rows the caller's points must be mapped to (ARD scaling or the camphor embedding)."""
        return self.scale is not None or self.camphor is not None


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


class VarianceProjection:
    """A projected variance operator of one Posterior (Engine.project_variance): the device matrix T = Q^T H and the
    ppbo_var_projection that names it.  rows == 0: no projection (the scoring entries then run their usual launches);
    otherwise 0 <= var - var_projected <= bound for every candidate, bound <= tol sigma_f^2."""

    def __init__(self, T, struct, tol):
        self.T, self.struct, self.tol = T, struct, float(tol)

    rows = property(lambda self: self.struct.rows)
    bound = property(lambda self: self.struct.bound)


class Engine:
    """One ppbo_ctx bound to one GPU."""

    def __init__(self, device: int = 0):
        if not torch.cuda.is_available():
            raise RuntimeError("ppbo_amd needs a ROCm GPU (torch.cuda.is_available() is False); there is no CPU path")
        self.lib = _lib.load()
        self.device = torch.device("cuda", device)   # every allocation / stream below names it explicitly
        ctx = C.c_void_p()
        rc = self.lib.ppbo_ctx_create(device, C.byref(ctx))
        if rc != 0:
            raise RuntimeError(f"ppbo_ctx_create failed with code {rc}")
        self.ctx = ctx

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.ppbo_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- helpers -------------------------------------------------------
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _err(self):
        buf = C.create_string_buffer(512)
        self.lib.ppbo_last_error(self.ctx, buf, 512)
        return buf.value.decode(errors="replace")

    def _check(self, rc, what, info=0):
        if rc == 0:
            return
        if rc == PPBO_ERR_NOT_PD:
            raise NotPositiveDefinite(f"{what}: {self._err()}", info)
        raise RuntimeError(f"{what} failed (code {rc}): {self._err()}")

    def dev(self, a, dtype=torch.float64):
        if isinstance(a, torch.Tensor):
            return a.to(device=self.device, dtype=dtype).contiguous()
        return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=self.device)

    def empty(self, *shape):
        return torch.empty(*shape, dtype=torch.float64, device=self.device)

    @staticmethod
    def _theta(theta):
        return (C.c_double * 3)(float(theta[0]), float(theta[1]), float(theta[2]))

    # ---- ARD: the one place that knows which coordinates the device works in ------------------------------------------
    @staticmethod
    def _dptr(a):
        return a.ctypes.data_as(C.POINTER(C.c_double))

    def scale_points(self, X, scale, out=None):
        """out = X * scale row-wise (ppbo_scale_points; out may be X itself)."""
        X = self.dev(X)
        M, D = X.shape
        sc = np.ascontiguousarray(np.asarray(scale, dtype=np.float64).reshape(-1))
        if sc.size != D:
            raise ValueError(f"scale_points: {sc.size} scales for {D} columns")
        out = self.empty(M, D) if out is None else out
        rc = self.lib.ppbo_scale_points(self.ctx, _ptr(X), M, D, self._dptr(sc), _ptr(out), self._stream())
        self._check(rc, "ppbo_scale_points")
        return out

    def camphor_embed(self, X, ls):
        """e(X) [M, 11] of the caller's rows X [M, 6] for the camphor length scales ls (ppbo_camphor_embed)."""
        X = self.dev(X)
        if X.dim() != 2 or X.shape[1] != 6:
            raise ValueError(f"camphor_embed: points of shape {tuple(X.shape)}, [M, 6] required")
        l = np.ascontiguousarray(ls, dtype=np.float64)
        out = self.empty(X.shape[0], 11)
        rc = self.lib.ppbo_camphor_embed(self.ctx, _ptr(X), X.shape[0], self._dptr(l), _ptr(out), self._stream())
        self._check(rc, "ppbo_camphor_embed")
        return out

    @staticmethod
    def _kid(kernel):
        """The device's kernel id: camphor_copper_ard_kernel is SE on embedded rows."""
        return KERNEL_IDS["SE_kernel" if kernel == CAMPHOR_ARD else kernel]

    def _ard(self, X, theta, kernel):
        """(rows the device works on, theta it sees, scale or None) for the caller's rows X and theta."""
        X = self.dev(X)
        if kernel == CAMPHOR_ARD:
            return self.camphor_embed(X, camphor_lengthscales(theta, X.shape[1])), (float(theta[0]), 1.0, float(theta[2])), None
        ls = lengthscales(theta, X.shape[1], kernel)
        if ls is None:
            return X, theta, None
        scale = 1.0 / ls
        return self.scale_points(X, scale), (float(theta[0]), 1.0, float(theta[2])), scale

    def _points(self, post: Posterior, Xc):
        """Points in the caller's coordinates -> the rows the posterior's device state is in."""
        Xc = self.dev(Xc)
        if not post.embedded:
            return Xc
        D = post.X.shape[1] if post.camphor is None else 6
        if Xc.dim() != 2 or Xc.shape[1] != D:
            raise ValueError(f"points of shape {tuple(Xc.shape)} for a model of {D} dimensions")
        if post.camphor is not None:
            return self.camphor_embed(Xc, post.camphor)
        return self.scale_points(Xc, post.scale)

    def _camphor_fields(self, X, theta, kernel):
        """The Posterior fields of a camphor_copper_ard_kernel model (its six length scales and a copy of the caller's
        rows), else {}."""
        if kernel != CAMPHOR_ARD:
            return {}
        X = self.dev(X)
        return dict(camphor=camphor_lengthscales(theta, X.shape[1]), Xc=X.clone())

    def mean_posterior(self, X, theta, kernel, m, alpha):
        """A Posterior usable for the mean only (alpha given, no variance state) at the caller's rows X."""
        Xd, _, scale = self._ard(X, theta, kernel)
        return Posterior(kernel, theta_key(theta), m, Xd, alpha, None, None, None, scale=scale,
                         **self._camphor_fields(X, theta, kernel))

    def _model(self, post: Posterior, with_var=True, kstar_fp32=False, projection=None):
        """projection: a VarianceProjection of `post` (project_variance) for the entries that read ppbo_model.proj."""
        N, D = post.X.shape
        md = _lib.Model()
        md.kernel_id = self._kid(post.kernel)
        md.N, md.D, md.m = N, D, post.m
        md.theta = self._theta(post.theta if not post.embedded else (post.theta[0], 1.0, post.theta[2]))
        md.d_X = post.X.data_ptr()
        md.d_alpha = post.alpha.data_ptr()
        md.d_lam_diag = post.lam_diag.data_ptr() if post.lam_diag is not None else 0
        md.d_lam_off = post.lam_off.data_ptr() if post.lam_off is not None else 0
        md.d_G = post.G.data_ptr() if (with_var and post.G is not None) else 0
        md.kstar_fp32 = int(bool(kstar_fp32))
        md.d_Gt = 0
        md.form = post.form
        # the coordinates post.X is in (ppbo_coords); md._coords keeps the host coefficients alive as long as md
        if post.camphor is not None:
            md._coords = _lib.coords(_lib.COORDS_CAMPHOR, post.camphor, post.Xc.data_ptr() if post.Xc is not None else None)
            md.coords = md._coords
        elif post.scale is not None:
            md._coords = _lib.coords(_lib.COORDS_SCALED, post.scale)
            md.coords = md._coords
        if projection is not None:
            # ppbo_model.proj, a copy of the struct; md._projection keeps T alive as long as md
            md._projection = projection
            md.proj = projection.struct
        if md.d_G and post.form == FORM_NODE and N <= 1024 and post.kernel != "camphor_copper_kernel":
            # models the one-launch scoring kernel takes: its matrix-core loop reads G transposed -- formed ONCE per
            # posterior here (the library would otherwise do it in a workspace on every call)
            if post.Gt is None or post.Gt.device != post.G.device:
                post.Gt = self.transposed_G(post.G)
                # once per posterior: the transpose is complete before ANY stream (another engine's, a side thread's) can
                # be handed the pointer through this Posterior
                torch.cuda.current_stream(self.device).synchronize()
            md.d_Gt = post.Gt.data_ptr()
        return md

    def project_variance(self, post: Posterior, tol=1e-10):
        """The variance contraction of `post` in a bounded low-rank basis (ppbo_var_projection_build), built once and cached
        on the posterior: a VarianceProjection with 0 <= var - var_projected <= tol sigma_f^2 for every candidate, or one
        with rows == 0 where the model takes none (node form, the one-launch kernel's shapes, tolerance not reached).
        Deterministic: every rank of a replicated fit builds the same bits."""
        cached = post.proj
        if cached is not None and cached.tol == float(tol) and cached.T.device == post.alpha.device:
            return cached
        md = self._model(post, True)
        rows, ld = C.c_int(0), C.c_int(0)
        self._check(self.lib.ppbo_var_projection_shape(C.byref(md), C.byref(rows), C.byref(ld)), "ppbo_var_projection_shape")
        T = self.empty(max(rows.value, 1), ld.value)
        st = _lib.VarProjection()
        rc = self.lib.ppbo_var_projection_build(self.ctx, C.byref(md), float(tol), _ptr(T), C.byref(st), self._stream())
        self._check(rc, "ppbo_var_projection_build")
        torch.cuda.current_stream(self.device).synchronize()      # complete before any other stream is handed T
        post.proj = VarianceProjection(T, st, tol)
        return post.proj

    def posterior_form(self, kernel, N, D, m):
        """The operator form to build for a model of this shape (ppbo_posterior_form): FORM_NODE where the one-launch
        scoring kernel takes the model, FORM_EDGE elsewhere.  D: the device's row width (embedded rows for camphor)."""
        rc = self.lib.ppbo_posterior_form(self.ctx, self._kid(kernel), int(N), int(D), int(m))
        if rc < 0:
            self._check(rc, "ppbo_posterior_form")
        return rc

    def transposed_G(self, G):
        """G [N, N] -> its transpose in the layout of ppbo_model.d_Gt (ppbo_transposed_G)."""
        N = G.shape[0]
        rows, ld = C.c_int(0), C.c_int(0)
        self._check(self.lib.ppbo_transposed_G_shape(N, C.byref(rows), C.byref(ld)), "ppbo_transposed_G_shape")
        Gt = self.empty(rows.value, ld.value)
        self._check(self.lib.ppbo_transposed_G(self.ctx, _ptr(G), N, _ptr(Gt), self._stream()), "ppbo_transposed_G")
        return Gt

    # ---- the path's collective behind the C-ABI (RCCL; no torch.distributed needed) -----------------
    def dist_unique_id(self) -> bytes:
        buf = C.create_string_buffer(128)
        self._check(self.lib.ppbo_dist_unique_id(self.ctx, buf), "ppbo_dist_unique_id")
        return buf.raw

    def dist_init(self, unique_id: bytes, rank: int, world: int):
        self._check(self.lib.ppbo_dist_init(self.ctx, C.c_char_p(unique_id), int(rank), int(world)), "ppbo_dist_init")

    def argmax_allgather(self, local_val: float, local_global_idx: int):
        bv, bi = C.c_double(0.0), C.c_int64(-1)
        rc = self.lib.ppbo_argmax_allgather(self.ctx, float(local_val), int(local_global_idx), C.byref(bv), C.byref(bi),
                                            self._stream())
        self._check(rc, "ppbo_argmax_allgather")
        return bv.value, bi.value

    def argmax_combine(self, records):
        """records: device float64 [world, 2] of (value, global index) -> (best value, its index); reduced on the
        device by one wavefront, one 16-byte read-back."""
        bv, bi = C.c_double(0.0), C.c_int64(-1)
        rc = self.lib.ppbo_argmax_combine(self.ctx, _ptr(records), int(records.numel() // 2), C.byref(bv), C.byref(bi),
                                          self._stream())
        self._check(rc, "ppbo_argmax_combine")
        return bv.value, bi.value

    def dist_destroy(self):
        self._check(self.lib.ppbo_dist_destroy(self.ctx), "ppbo_dist_destroy")

    def argmax_allgather_record(self, record):
        """record: device float64 [2] as written by predict_record -> job-wide (best value, global index) through the
        ctx's RCCL communicator (ppbo_argmax_allgather_record: all-gather, reduction, one 16-byte read-back)."""
        bv, bi = C.c_double(0.0), C.c_int64(-1)
        rc = self.lib.ppbo_argmax_allgather_record(self.ctx, _ptr(record), C.byref(bv), C.byref(bi), self._stream())
        self._check(rc, "ppbo_argmax_allgather_record")
        return bv.value, bi.value

    def predict_record(self, post, Xc, score=SCORE_MEAN, mustar=0.0, index_offset=0, out=None, kstar_fp32=False,
                       projection=None):
        """One shard of a sharded search, enqueue only (ppbo_predict_record): out[2] (device) = (best score,
        index_offset + first row index as a float64); nothing is read back, nothing synchronises.  projection: as predict's."""
        Xc = self.dev(Xc)
        Xc = self._points(post, Xc)
        md = self._model(post, score != SCORE_MEAN, kstar_fp32, projection)
        rec = self.empty(2) if out is None else out
        rc = self.lib.ppbo_predict_record(self.ctx, C.byref(md), _ptr(Xc), Xc.shape[0], int(score), float(mustar),
                                          int(index_offset), _ptr(rec), self._stream())
        self._check(rc, "ppbo_predict_record")
        return rec

    def prune_report(self, post, Xc, score, mustar=0.0, projection=None):
        """What the pruned search decides for one chunk of candidates (ppbo_predict_prune_report; at most 65536 rows, an
        edge-form posterior on the three-launch path, SCORE_POINTWISE_EI or SCORE_VARIANCE): device tensors u2 (>= the
        contraction's sum of squares), s_lo, s_hi per candidate, and threshold, n_surv, pruned."""
        Xc = self._points(post, self.dev(Xc))
        M = Xc.shape[0]
        md = self._model(post, True, projection=projection)
        u2, lo, hi = self.empty(M), self.empty(M), self.empty(M)
        thr, ns, pr = C.c_double(0.0), C.c_int(0), C.c_int(0)
        rc = self.lib.ppbo_predict_prune_report(self.ctx, C.byref(md), _ptr(Xc), M, int(score), float(mustar),
                                                _ptr(u2), _ptr(lo), _ptr(hi), C.byref(thr), C.byref(ns), C.byref(pr),
                                                self._stream())
        self._check(rc, "ppbo_predict_prune_report")
        return dict(u2=u2, s_lo=lo, s_hi=hi, threshold=thr.value, n_surv=ns.value, pruned=pr.value)

    def search_sharded(self, post, Xc, score=SCORE_MEAN, mustar=0.0, index_offset=0, kstar_fp32=False, projection=None):
        """One whole sharded search step in ONE library call (ppbo_search_sharded): score this rank's rows, RCCL
        all-gather of the 16-byte records (when dist_init has run on this ctx), reduction, one read-back.  Not for a
        camphor_copper_ard_kernel posterior.  projection: as predict's."""
        if post.camphor is not None:
            raise ValueError("search_sharded does not take a camphor_copper_ard_kernel posterior")
        Xc = self._points(post, Xc)
        md = self._model(post, score != SCORE_MEAN, kstar_fp32, projection)
        bv, bi = C.c_double(0.0), C.c_int64(-1)
        rc = self.lib.ppbo_search_sharded(self.ctx, C.byref(md), _ptr(Xc), Xc.shape[0], int(score), float(mustar),
                                          int(index_offset), C.byref(bv), C.byref(bi), self._stream())
        self._check(rc, "ppbo_search_sharded")
        return bv.value, bi.value

    # ---- per-kernel event timing ---------------------------------------------
    def profile(self, on=True):
        self.lib.ppbo_profile_enable(self.ctx, int(on))
        self.lib.ppbo_profile_reset(self.ctx)

    def profile_reset(self):
        self.lib.ppbo_profile_reset(self.ctx)

    def profile_read(self, name):
        tot, cnt = C.c_double(0.0), C.c_int(0)
        rc = self.lib.ppbo_profile_read(self.ctx, name.encode(), C.byref(tot), C.byref(cnt))
        self._check(rc, "ppbo_profile_read")
        return tot.value, cnt.value

    # ---- K1 / K2 --------------------------------------------------------
    def gram(self, X, theta, kernel="SE_kernel", shrink=SHRINKAGE, out=None):
        X, theta, _ = self._ard(X, theta, kernel)
        N, D = X.shape
        S = self.empty(N, N) if out is None else out
        rc = self.lib.ppbo_gram(self.ctx, self._kid(kernel), _ptr(X), N, D, self._theta(theta), shrink, _ptr(S),
                                self._stream())
        self._check(rc, "ppbo_gram")
        return S

    def store_floor(self, out):
        """Write-only pass over an N x N device matrix (ppbo_store_floor): the Gram kernel's ceiling at that N."""
        rc = self.lib.ppbo_store_floor(self.ctx, _ptr(out), out.shape[0], self._stream())
        self._check(rc, "ppbo_store_floor")
        return out

    def cross_cov(self, X1, X2, theta, kernel="SE_kernel"):
        X1, th, scale = self._ard(X1, theta, kernel)
        if kernel == CAMPHOR_ARD:
            X2 = self._ard(X2, theta, kernel)[0]
        else:
            X2 = self.dev(X2) if scale is None else self.scale_points(X2, scale)
        theta = th
        n1, D = X1.shape
        n2 = X2.shape[0]
        K = self.empty(n1, n2)
        rc = self.lib.ppbo_cross_cov(self.ctx, self._kid(kernel), _ptr(X1), n1, _ptr(X2), n2, D, self._theta(theta),
                                     _ptr(K), n2, self._stream())
        self._check(rc, "ppbo_cross_cov")
        return K

    # ---- K6 ----------------------------------------------------------------
    def potrf_(self, A):
        """In-place lower Cholesky of a square device tensor."""
        N = A.shape[0]
        info = C.c_int(0)
        rc = self.lib.ppbo_potrf(self.ctx, _ptr(A), N, A.stride(0), C.byref(info), self._stream())
        self._check(rc, "ppbo_potrf", info.value)
        return A

    def pd_inverse(self, A):
        A = self.dev(A)
        N = A.shape[0]
        out = self.empty(N, N)
        info = C.c_int(0)
        rc = self.lib.ppbo_pd_inverse(self.ctx, _ptr(A), N, _ptr(out), C.byref(info), self._stream())
        self._check(rc, "ppbo_pd_inverse", info.value)
        return out

    def pd_inverse_factors(self, A):
        """(A^-1, L^-1) with A = L L^T: what pd_inverse_append borders."""
        A = self.dev(A)
        N = A.shape[0]
        out, linv = self.empty(N, N), self.empty(N, N)
        info = C.c_int(0)
        rc = self.lib.ppbo_pd_inverse_factors(self.ctx, _ptr(A), N, _ptr(out), _ptr(linv), C.byref(info), self._stream())
        self._check(rc, "ppbo_pd_inverse_factors", info.value)
        return out, linv

    def pd_inverse_chol(self, A):
        """(A^-1, L) with A = L L^T (lower triangle of L valid): what fit_fmap_whitened iterates with."""
        A = self.dev(A)
        N = A.shape[0]
        out, L = self.empty(N, N), self.empty(N, N)
        info = C.c_int(0)
        rc = self.lib.ppbo_pd_inverse_ex(self.ctx, _ptr(A), N, _ptr(out), _ptr(L), None, C.byref(info), self._stream())
        self._check(rc, "ppbo_pd_inverse_ex", info.value)
        return out, L

    def pd_inverse_factors3(self, A):
        """(A^-1, L^-1, L): everything the bordered append extends."""
        A = self.dev(A)
        N = A.shape[0]
        out, linv, L = self.empty(N, N), self.empty(N, N), self.empty(N, N)
        info = C.c_int(0)
        rc = self.lib.ppbo_pd_inverse_ex(self.ctx, _ptr(A), N, _ptr(out), _ptr(L), _ptr(linv), C.byref(info), self._stream())
        self._check(rc, "ppbo_pd_inverse_ex", info.value)
        return out, linv, L

    def pd_inverse_append(self, A, A11inv, L11inv, L11=None):
        """(A^-1, L^-1) of A[N,N] given those of its leading N1 x N1 block (one appended query, f-4); with L11 (the
        factor of that block) the bordered factor L comes back as a third result."""
        A, A11inv, L11inv = self.dev(A), self.dev(A11inv), self.dev(L11inv)
        N, N1 = A.shape[0], A11inv.shape[0]
        out, linv = self.empty(N, N), self.empty(N, N)
        info = C.c_int(0)
        if L11 is None:
            rc = self.lib.ppbo_pd_inverse_append(self.ctx, _ptr(A), N, _ptr(A11inv), _ptr(L11inv), N1, _ptr(out),
                                                 _ptr(linv), C.byref(info), self._stream())
            self._check(rc, "ppbo_pd_inverse_append", info.value)
            return out, linv
        L11 = self.dev(L11)
        L = self.empty(N, N)
        rc = self.lib.ppbo_pd_inverse_append_ex(self.ctx, _ptr(A), N, _ptr(A11inv), _ptr(L11inv), _ptr(L11), N1, _ptr(out),
                                                _ptr(linv), _ptr(L), C.byref(info), self._stream())
        self._check(rc, "ppbo_pd_inverse_append_ex", info.value)
        return out, linv, L

    def dgemm(self, A, B, transA=False, transB=False, alpha=1.0, beta=0.0, C_out=None):
        A, B = self.dev(A), self.dev(B)
        M = A.shape[1] if transA else A.shape[0]
        K = A.shape[0] if transA else A.shape[1]
        Nn = B.shape[0] if transB else B.shape[1]
        Cc = C_out if C_out is not None else self.empty(M, Nn)
        rc = self.lib.ppbo_dgemm(self.ctx, int(transA), int(transB), M, Nn, K, alpha, _ptr(A), A.stride(0), _ptr(B),
                                 B.stride(0), beta, _ptr(Cc), Cc.stride(0), self._stream())
        self._check(rc, "ppbo_dgemm")
        return Cc

    def lu_slogdet_(self, A):
        """LU with partial pivoting in place; returns (prod sign(u_ii), sum log|u_ii|)."""
        N = A.shape[0]
        sg, ld, info = C.c_double(0.0), C.c_double(0.0), C.c_int(0)
        rc = self.lib.ppbo_lu_slogdet(self.ctx, _ptr(A), N, A.stride(0), C.byref(sg), C.byref(ld), C.byref(info),
                                      self._stream())
        self._check(rc, "ppbo_lu_slogdet")
        return sg.value, ld.value, info.value

    def laplace_logdet(self, Sigma, lam_diag, lam_off, m):
        N = Sigma.shape[0]
        sg, ld, info = C.c_double(0.0), C.c_double(0.0), C.c_int(0)
        rc = self.lib.ppbo_laplace_logdet(self.ctx, _ptr(Sigma), _ptr(lam_diag), _ptr(lam_off), N, m, C.byref(sg),
                                          C.byref(ld), C.byref(info), self._stream())
        self._check(rc, "ppbo_laplace_logdet")
        return sg.value, ld.value, info.value

    def evidence_grad(self, X, theta, kernel, Sigma, Sigma_inv, fMAP, lam_diag, lam_off, m, shrink=SHRINKAGE):
        """ppbo_evidence_grad at one evidence's state (X and theta in the caller's coordinates; Sigma, Sigma^-1, f_MAP and
        the star-form Lambda(f_MAP) as the evidence formed them).  Returns (s_U, log|det A|, sums[D + 1], info) with the
        sign and log-determinant bit-identical to laplace_logdet; sums as include/ppbo_hip.h defines them, for the rows
        the device works on (scaled by 1 / l for per-dimension length scales; camphor_copper_ard_kernel: the 11 embedded
        columns).  Raises ValueError for a kernel outside ARD_KERNELS and NotPositiveDefinite (info = 2) when
        Sigma^-1 - Lambda is not positive definite."""
        if kernel not in ARD_KERNELS:
            raise ValueError(f"the evidence gradient is defined for the kernels {ARD_KERNELS}, not {kernel}")
        Xd, th, _ = self._ard(X, theta, kernel)
        N, D = Xd.shape
        f = self.dev(fMAP).reshape(-1)
        sg, ld, info = C.c_double(0.0), C.c_double(0.0), C.c_int(0)
        sums = np.zeros(D + 1)
        rc = self.lib.ppbo_evidence_grad(self.ctx, self._kid(kernel), _ptr(Xd), N, D, self._theta(th), float(shrink), int(m),
                                         _ptr(Sigma), _ptr(Sigma_inv), _ptr(f), _ptr(lam_diag), _ptr(lam_off), C.byref(sg),
                                         C.byref(ld), self._dptr(sums), C.byref(info), self._stream())
        self._check(rc, "ppbo_evidence_grad", info.value)
        return sg.value, ld.value, sums, info.value

    def dgemv(self, A, x, trans=False, lower=False):
        A, x = self.dev(A), self.dev(x).reshape(-1)
        N = A.shape[0]
        if A.dim() != 2 or A.shape[1] != N or x.numel() != N:
            raise ValueError(f"dgemv: A is {tuple(A.shape)}, x has {x.numel()} entries (a square A and len(x) == N are required)")
        y = self.empty(N)
        rc = self.lib.ppbo_dgemv(self.ctx, int(trans), int(lower), N, _ptr(A), A.stride(0), _ptr(x), _ptr(y),
                                 self._stream())
        self._check(rc, "ppbo_dgemv")
        return y

    # ---- K5 / fit -------------------------------------------------------------
    def laplace_terms(self, f, m, sigma):
        f = self.dev(f).reshape(-1)
        N = f.numel()
        T = self.empty(1)
        beta, ld, lo = self.empty(N), self.empty(N), self.empty(N)
        rc = self.lib.ppbo_laplace_terms(self.ctx, _ptr(f), N, m, float(sigma), _ptr(T), _ptr(beta), _ptr(ld),
                                         _ptr(lo), self._stream())
        self._check(rc, "ppbo_laplace_terms")
        return float(T.item()), beta, ld, lo

    def sum_phi(self, f, m, sigma, order):
        """Per-query sums of src/gp_model.py:206-218 (device tensor [N / (m+1)])."""
        f = self.dev(f).reshape(-1)
        N = f.numel()
        out = self.empty(N // (m + 1))
        rc = self.lib.ppbo_sum_phi(self.ctx, _ptr(f), N, m, float(sigma), int(order), _ptr(out), self._stream())
        self._check(rc, "ppbo_sum_phi")
        return out

    def regularize_covariance(self, K, reg_level=1e-4, pos_diag=True, jitter=1e-7):
        """src/misc.py:71-88 on a device copy of K (the caller's matrix is left alone, as the reference's callers
        use the returned value)."""
        K = self.dev(K).clone()
        N = K.shape[0]
        rc = self.lib.ppbo_regularize_covariance(self.ctx, _ptr(K), N, K.stride(0), float(reg_level), int(bool(pos_diag)),
                                                 float(jitter), self._stream())
        self._check(rc, "ppbo_regularize_covariance")
        return K

    def T_and_grad(self, Sigma_inv, f, m, sigma):
        f = self.dev(f).reshape(-1)
        N = f.numel()
        grad = self.empty(N)
        T = C.c_double(0.0)
        rc = self.lib.ppbo_T_and_grad(self.ctx, _ptr(Sigma_inv), _ptr(f), N, m, float(sigma), C.byref(T), _ptr(grad),
                                      self._stream())
        self._check(rc, "ppbo_T_and_grad")
        return T.value, grad

    def fit_fmap(self, Sigma_inv, f_init, m, sigma, gtol=1e-4, maxiter=0, verbose=False, initial_radius=0.0, L=None,
                 lbfgs_max_evals=0):
        """f_MAP from one start vector.  L = None: trust-region Newton on f (ppbo_fit_fmap, the reference's
        algorithm class); L = Cholesky factor of Sigma: whitened L-BFGS finished by that trust region
        (ppbo_fit_fmap_whitened) -- same optimum, tens of O(N^2) evaluations instead of O(N^3) factorizations."""
        f0 = self.dev(f_init).reshape(-1)
        N = f0.numel()
        out = self.empty(N)
        opts = _lib.FitOpts(float(gtol), int(maxiter), int(verbose), float(initial_radius), int(lbfgs_max_evals), 0, 0)
        st = _lib.FitStats()
        if L is None:
            rc = self.lib.ppbo_fit_fmap(self.ctx, _ptr(Sigma_inv), N, m, float(sigma), _ptr(f0), C.byref(opts),
                                        _ptr(out), C.byref(st), self._stream())
            self._check(rc, "ppbo_fit_fmap")
        else:
            rc = self.lib.ppbo_fit_fmap_whitened(self.ctx, _ptr(L), L.stride(0), _ptr(Sigma_inv), N, m, float(sigma),
                                                 _ptr(f0), C.byref(opts), _ptr(out), C.byref(st), self._stream())
            self._check(rc, "ppbo_fit_fmap_whitened")
        stats = dict(iterations=st.iterations, n_cholesky=st.n_cholesky, converged=bool(st.converged), T=st.T,
                     gradnorm=st.gradnorm, lbfgs_iterations=st.lbfgs_iterations, lbfgs_evals=st.lbfgs_evals,
                     lbfgs_status=st.lbfgs_status)
        return out, stats

    def gp_fit(self, X, theta, kernel, m, f_init, shrink=SHRINKAGE, gtol=1e-4, maxiter=0, verbose=0, lbfgs_max_evals=0,
               start_is_whitened=False, want_Sigma=True, want_Linv=False, want_posterior=True, form=None):
        """One whole GP fit in one library call (ppbo_gp_fit): Sigma, its Cholesky factor and inverse, f_MAP from one
        start by the whitened search, and the posterior state -- the work of update_Sigma + update_Sigma_inv +
        update_fMAP + the posterior (src/gp_model.py:91-117), everything enqueued behind each other on one stream with
        ONE host wait.  start_is_whitened: f_init holds z0 and the start is the prior draw L z0.
        Returns dict(Sigma, Sigma_inv, L, Linv, fMAP, post, stats, info); info = 2 (with post = None) when
        Sigma^-1 - Lambda_MAP is not positive definite (raises NotPositiveDefinite when Sigma itself is not).
        form: the posterior's operator form (None: posterior_form's choice for this shape)."""
        key = theta_key(theta)
        cam = self._camphor_fields(X, theta, kernel)
        X, theta, scale = self._ard(X, theta, kernel)
        N, D = X.shape
        if form is None:
            form = self.posterior_form(kernel, N, D, m)
        f0 = self.dev(f_init).reshape(-1)
        if f0.numel() != N:
            raise ValueError(f"gp_fit: the start vector has {f0.numel()} entries, the design {N} rows")
        Sigma = self.empty(N, N) if want_Sigma else None
        Sinv, L = self.empty(N, N), self.empty(N, N)
        Linv = self.empty(N, N) if want_Linv else None
        fmap = self.empty(N)
        if want_posterior:
            alpha, ld, lo, G = self.empty(N), self.empty(N), self.empty(N), self.empty(N, N)
        else:
            alpha = ld = lo = G = None
        opts = _lib.FitOpts(float(gtol), int(maxiter), int(verbose), 0.0, int(lbfgs_max_evals), 0, int(bool(start_is_whitened)))
        st = _lib.FitStats()
        info = C.c_int(0)
        rc = self.lib.ppbo_gp_fit(self.ctx, self._kid(kernel), _ptr(X), N, D, self._theta(theta), float(shrink), int(m),
                                  _ptr(f0), C.byref(opts), _ptr(Sigma), _ptr(Sinv), _ptr(L), _ptr(Linv), _ptr(fmap),
                                  _ptr(alpha), _ptr(ld), _ptr(lo), _ptr(G), int(form), C.byref(st), C.byref(info),
                                  self._stream())
        if rc == PPBO_ERR_NOT_PD and info.value == 2:
            post = None
        else:
            self._check(rc, "ppbo_gp_fit", info.value)
            post = Posterior(kernel, key, m, X, alpha, ld, lo, G, None, scale=scale, form=form,
                             **cam) if want_posterior else None
        stats = dict(iterations=st.iterations, n_cholesky=st.n_cholesky, converged=bool(st.converged), T=st.T,
                     gradnorm=st.gradnorm, lbfgs_iterations=st.lbfgs_iterations, lbfgs_evals=st.lbfgs_evals,
                     lbfgs_status=st.lbfgs_status)
        return dict(Sigma=Sigma, Sigma_inv=Sinv, L=L, Linv=Linv, fMAP=fmap, post=post, stats=stats, info=info.value)

    def posterior(self, X, theta, kernel, Sigma_inv, fMAP, m, want_P=False, form=None) -> Posterior:
        """form: FORM_NODE / FORM_EDGE, None: posterior_form's choice for this shape."""
        key = theta_key(theta)
        cam = self._camphor_fields(X, theta, kernel)
        X, _, scale = self._ard(X, theta, kernel)
        f = self.dev(fMAP).reshape(-1)
        N = f.numel()
        if form is None:
            form = self.posterior_form(kernel, N, X.shape[1], m)
        alpha, ld, lo = self.empty(N), self.empty(N), self.empty(N)
        G = self.empty(N, N)
        P = self.empty(N, N) if want_P else None
        info = C.c_int(0)
        rc = self.lib.ppbo_posterior(self.ctx, _ptr(Sigma_inv), _ptr(f), N, m, float(theta[0]), _ptr(alpha), _ptr(ld),
                                     _ptr(lo), _ptr(G), _ptr(P), int(form), C.byref(info), self._stream())
        self._check(rc, "ppbo_posterior", info.value)
        return Posterior(kernel, key, m, X, alpha, ld, lo, G, P, scale=scale, form=form, **cam)

    # ---- prediction ---------------------------------------------------------------
    def predict(self, post: Posterior, Xc, score=SCORE_MEAN, mustar=0.0, want_mu=True, want_var=True,
                want_score=False, want_best=True, kstar_fp32=False, projection=None):
        """projection: a VarianceProjection of `post` (project_variance) to contract the variance with, or None."""
        Xc = self._points(post, Xc)
        M = Xc.shape[0]
        with_var = want_var or score != SCORE_MEAN
        md = self._model(post, with_var, kstar_fp32, projection)
        mu = self.empty(M) if want_mu else None
        var = self.empty(M) if (want_var and with_var) else None
        sc = self.empty(M) if want_score else None
        bv, bi = C.c_double(0.0), C.c_int64(-1)
        rc = self.lib.ppbo_predict(self.ctx, C.byref(md), _ptr(Xc), M, int(score), float(mustar), _ptr(mu), _ptr(var),
                                   _ptr(sc), C.byref(bv) if want_best else None, C.byref(bi) if want_best else None,
                                   self._stream())
        self._check(rc, "ppbo_predict")
        return dict(mu=mu, var=var, score=sc, best_val=bv.value, best_idx=bi.value)

    @staticmethod
    def _pair_shapes(post: Posterior, Xa, Xb, what="predict_pairs", sets="the two sides", rows="pairs"):
        """The refusals of predict_pairs / predict_slopes that shapes alone decide (before anything reaches the device):
        returns M."""
        sa, sb = tuple(np.shape(Xa)), tuple(np.shape(Xb))
        D = 6 if post.camphor is not None else post.X.shape[1]
        if len(sa) != 2 or sa != sb:
            raise ValueError(f"{what}: {sets} have shapes {sa} and {sb}; two equal [M, D] sets are required")
        if sa[1] != D:
            raise ValueError(f"{what}: points of width {sa[1]} for a model of {D} dimensions")
        if sa[0] < 1:
            raise ValueError(f"{what}: no {rows}")
        return sa[0]

    def predict_pairs(self, post: Posterior, Xa, Xb, score=PAIR_PROB, want_mu=True, want_var=True, want_prob=True,
                      want_score=False, want_best=True):
        """Duels (ppbo_predict_pairs): for the M pairs (Xa[i], Xb[i]) in the caller's coordinates the posterior mean and
        variance of f(a) - f(b) and p = P(a > b), as device tensors mu / var / prob / score (None where not asked for),
        with best_val / best_idx = the largest score (the quantity `score` names) and its first row.  PAIR_MEAN without
        var and prob needs no variance operator."""
        M = self._pair_shapes(post, Xa, Xb)
        if score not in (PAIR_MEAN, PAIR_VARIANCE, PAIR_PROB):
            raise ValueError(f"predict_pairs: unknown score kind {score}")
        Xa, Xb = self._points(post, Xa), self._points(post, Xb)
        with_var = want_var or want_prob or score != PAIR_MEAN
        md = self._model(post, with_var)
        mu = self.empty(M) if want_mu else None
        var = self.empty(M) if want_var else None
        pr = self.empty(M) if want_prob else None
        sc = self.empty(M) if want_score else None
        bv, bi = C.c_double(0.0), C.c_int64(-1)
        rc = self.lib.ppbo_predict_pairs(self.ctx, C.byref(md), _ptr(Xa), _ptr(Xb), M, int(score), _ptr(mu), _ptr(var),
                                         _ptr(pr), _ptr(sc), C.byref(bv) if want_best else None,
                                         C.byref(bi) if want_best else None, self._stream())
        self._check(rc, "ppbo_predict_pairs")
        return dict(mu=mu, var=var, prob=pr, score=sc, best_val=bv.value, best_idx=bi.value)

    def _directions(self, post: Posterior, X, Xi):
        """Directions in the caller's coordinates -> the coordinates the posterior's device state is in: the Jacobian of
        _points' map at X applied to Xi (ARD: s (.) xi; camphor_copper_ard_kernel: J_e(x) xi, formed on the host)."""
        if post.camphor is not None:
            to_host = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)  # noqa: E731
            return self.dev(camphor_embed_directions(to_host(X), to_host(Xi), post.camphor))
        Xi = self.dev(Xi)
        return Xi if post.scale is None else self.scale_points(Xi, post.scale)

    def predict_slopes(self, post: Posterior, X, Xi, score=SLOPE_PROB, want_mu=True, want_var=True, want_prob=True,
                       want_score=False, want_best=True):
        """Slopes (ppbo_predict_slopes): for the M rows (X[i], Xi[i]) in the caller's coordinates the posterior mean and
        variance of d/da f(x + a xi) at a = 0 and p = P(slope > 0), as device tensors mu / var / prob / score (None where
        not asked for), with best_val / best_idx = the largest score (the quantity `score` names) and its first row.
        SLOPE_MEAN without var and prob needs no variance operator."""
        M = self._pair_shapes(post, X, Xi, "predict_slopes", "points and directions", "rows")
        if score not in (SLOPE_MEAN, SLOPE_VARIANCE, SLOPE_PROB):
            raise ValueError(f"predict_slopes: unknown score kind {score}")
        Xi = self._directions(post, X, Xi)
        X = self._points(post, X)
        with_var = want_var or want_prob or score != SLOPE_MEAN
        md = self._model(post, with_var)
        mu = self.empty(M) if want_mu else None
        var = self.empty(M) if want_var else None
        pr = self.empty(M) if want_prob else None
        sc = self.empty(M) if want_score else None
        bv, bi = C.c_double(0.0), C.c_int64(-1)
        rc = self.lib.ppbo_predict_slopes(self.ctx, C.byref(md), _ptr(X), _ptr(Xi), M, int(score), _ptr(mu), _ptr(var),
                                          _ptr(pr), _ptr(sc), C.byref(bv) if want_best else None,
                                          C.byref(bi) if want_best else None, self._stream())
        self._check(rc, "ppbo_predict_slopes")
        return dict(mu=mu, var=var, prob=pr, score=sc, best_val=bv.value, best_idx=bi.value)

    @staticmethod
    def _gradient_shapes(post: Posterior, X, score):
        """The refusals of predict_gradients that shapes alone decide (before anything reaches the device): returns M."""
        sx = tuple(np.shape(X))
        D = 6 if post.camphor is not None else post.X.shape[1]
        if len(sx) != 2:
            raise ValueError(f"predict_gradients: points of shape {sx}; one [M, D] set is required")
        if sx[1] != D:
            raise ValueError(f"predict_gradients: points of width {sx[1]} for a model of {D} dimensions")
        if sx[0] < 1:
            raise ValueError("predict_gradients: no points")
        if score not in (GRAD_NONE, GRAD_TRACE, GRAD_NORM2):
            raise ValueError(f"predict_gradients: unknown score kind {score}")
        return sx[0]

    def predict_gradients(self, post: Posterior, X, score=GRAD_NONE, want_mean=True, want_cov=True, want_score=False,
                          want_best=True):
        """Gradients (ppbo_predict_gradients): for the M points X[i] in the caller's coordinates the posterior of the
        whole gradient, grad f(x) ~ N(mean, cov), as device tensors mean [M, D] and cov [M, D, D] (symmetric bit for bit;
        None where not asked for), with score [M] = GRAD_TRACE: tr C, GRAD_NORM2: E |grad f|^2 = |m|^2 + tr C, and
        best_val / best_idx = the largest score and its first row ((NaN, -1) with GRAD_NONE).  Everything is in the
        caller's coordinates: an ARD model's m <- s (.) m, C <- S C S and the metric s^2; a camphor_copper_ard_kernel
        model is pulled back from the embedding's 11 columns by its Jacobian (J'm, J'CJ) and scored here.  The mean alone
        (want_cov = False, GRAD_NONE) needs no variance operator."""
        M = self._gradient_shapes(post, X, score)
        scored = score != GRAD_NONE
        with_var = want_cov or scored
        cam = post.camphor is not None
        Xc = self.dev(X)
        Xd = self._points(post, Xc)
        D = Xd.shape[1]
        md = self._model(post, with_var)
        need_mean = want_mean or (cam and score == GRAD_NORM2)
        mean = self.empty(M, D) if need_mean else None
        cov = self.empty(M, D, D) if (want_cov or (cam and scored)) else None
        sc = self.empty(M) if (want_score and not cam) else None
        metric = None
        if post.scale is not None:
            metric = np.ascontiguousarray(np.asarray(post.scale, dtype=np.float64) ** 2)
        bv, bi = C.c_double(float("nan")), C.c_int64(-1)
        lib_best = want_best and scored and not cam
        rc = self.lib.ppbo_predict_gradients(self.ctx, C.byref(md), _ptr(Xd), M, self._dptr(metric) if metric is not None else None,
                                             GRAD_NONE if cam else int(score), _ptr(mean), _ptr(cov), _ptr(sc),
                                             C.byref(bv) if lib_best else None, C.byref(bi) if lib_best else None,
                                             self._stream())
        self._check(rc, "ppbo_predict_gradients")
        best_val, best_idx = bv.value, bi.value
        if post.scale is not None:
            s = self.dev(post.scale)
            if mean is not None:
                mean = mean * s
            if cov is not None:
                cov = cov * torch.outer(s, s)          # (s_d s_e = s_e s_d: the symmetry survives bit for bit)
        elif cam:
            mean, cov = camphor_pull_back(Xc, post.camphor, mean, cov)
            if scored:
                sc = torch.diagonal(cov, dim1=1, dim2=2).sum(dim=1)
                if score == GRAD_NORM2:
                    sc = sc + (mean * mean).sum(dim=1)
                if want_best:
                    ok = ~torch.isnan(sc)
                    if bool(ok.any()):
                        best_val = float(sc[ok].max())
                        best_idx = int(torch.nonzero(ok & (sc == best_val))[0, 0])
                if not want_score:
                    sc = None
            if not want_mean:
                mean = None
            if not want_cov:
                cov = None
        return dict(mean=mean, cov=cov, score=sc, best_val=best_val, best_idx=best_idx)

    def predict_curvatures(self, post: Posterior, X, Xi, score=CURV_PROB, want_mu=True, want_var=True, want_prob=True,
                           want_score=False, want_best=True):
        """Curvatures (ppbo_predict_curvatures): for the M rows (X[i], Xi[i]) in the caller's coordinates the posterior
        mean and variance of d^2/da^2 f(x + a xi) at a = 0 and p = P(curvature < 0), as device tensors mu / var / prob /
        score (None where not asked for), with best_val / best_idx = the largest score (the quantity `score` names) and
        its first row.  CURV_MEAN without var and prob needs no variance operator.  A Matern-3/2 posterior is refused:
        the curvature of its sample paths has no finite variance.  camphor_copper_ard_kernel: the line x + a xi is a
        curved path in the embedding, whose acceleration is formed on the host and passed as d_Xa."""
        M = self._pair_shapes(post, X, Xi, "predict_curvatures", "points and directions", "rows")
        if score not in (CURV_MEAN, CURV_VARIANCE, CURV_PROB):
            raise ValueError(f"predict_curvatures: unknown score kind {score}")
        if post.kernel == "Matern32_kernel":
            raise ValueError("predict_curvatures: no curvature for Matern32_kernel (its sample paths are differentiable once only)")
        Xa = None
        if post.camphor is not None:
            to_host = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)  # noqa: E731
            Xa = self.dev(camphor_embed_accelerations(to_host(X), to_host(Xi), post.camphor))
        Xi = self._directions(post, X, Xi)
        X = self._points(post, X)
        with_var = want_var or want_prob or score != CURV_MEAN
        md = self._model(post, with_var)
        mu = self.empty(M) if want_mu else None
        var = self.empty(M) if want_var else None
        pr = self.empty(M) if want_prob else None
        sc = self.empty(M) if want_score else None
        bv, bi = C.c_double(0.0), C.c_int64(-1)
        rc = self.lib.ppbo_predict_curvatures(self.ctx, C.byref(md), _ptr(X), _ptr(Xi), _ptr(Xa), M, int(score), _ptr(mu),
                                              _ptr(var), _ptr(pr), _ptr(sc), C.byref(bv) if want_best else None,
                                              C.byref(bi) if want_best else None, self._stream())
        self._check(rc, "ppbo_predict_curvatures")
        return dict(mu=mu, var=var, prob=pr, score=sc, best_val=bv.value, best_idx=bi.value)

    @staticmethod
    def _functional_shapes(post: Posterior, Xg, w):
        """The refusals of predict_functionals that shapes alone decide (before anything reaches the device): returns
        (M, G, w_stride)."""
        sx, sw = tuple(np.shape(Xg)), tuple(np.shape(w))
        D = 6 if post.camphor is not None else post.X.shape[1]
        if len(sx) != 3:
            raise ValueError(f"predict_functionals: groups of shape {sx}; an [M, G, D] set is required")
        M, G = sx[0], sx[1]
        if sx[2] != D:
            raise ValueError(f"predict_functionals: points of width {sx[2]} for a model of {D} dimensions")
        if M < 1:
            raise ValueError("predict_functionals: no groups")
        if G < 1 or G > FUNCTIONAL_MAX_G:
            raise ValueError(f"predict_functionals: {G} points per group (1 .. {FUNCTIONAL_MAX_G})")
        if sw != (G,) and sw != (M, G):
            raise ValueError(f"predict_functionals: weights of shape {sw} for groups of shape {sx}; [G] or [M, G] is required")
        return M, G, (G if len(sw) == 2 else 0)

    def predict_functionals(self, post: Posterior, Xg, w, threshold=0.0, score=FUNCTIONAL_PROB, want_mu=True,
                            want_var=True, want_prob=True, want_score=False, want_best=True):
        """Averages and contrasts (ppbo_predict_functionals): for the M groups Xg[i] of G points in the caller's
        coordinates and the weights w ([G]: one row for all groups, or [M, G]) the posterior mean and variance of
        L f = sum_g w[g] f(Xg[i, g]) and p = P(L f > threshold), as device tensors mu / var / prob / score (None where not
        asked for), with best_val / best_idx = the largest score (the quantity `score` names) and its first group.
        FUNCTIONAL_MEAN without var and prob needs no variance operator."""
        M, G, w_stride = self._functional_shapes(post, Xg, w)
        if score not in (FUNCTIONAL_MEAN, FUNCTIONAL_VARIANCE, FUNCTIONAL_PROB):
            raise ValueError(f"predict_functionals: unknown score kind {score}")
        if not np.isfinite(float(threshold)):
            raise ValueError(f"predict_functionals: threshold {threshold} is not finite")
        Xg = self.dev(Xg)
        Xg = self._points(post, Xg.reshape(M * G, Xg.shape[2]))      # [M G, the model's D], group-major
        w = self.dev(w)
        with_var = want_var or want_prob or score != FUNCTIONAL_MEAN
        md = self._model(post, with_var)
        mu = self.empty(M) if want_mu else None
        var = self.empty(M) if want_var else None
        pr = self.empty(M) if want_prob else None
        sc = self.empty(M) if want_score else None
        bv, bi = C.c_double(0.0), C.c_int64(-1)
        rc = self.lib.ppbo_predict_functionals(self.ctx, C.byref(md), _ptr(Xg), _ptr(w), int(w_stride), M, int(G),
                                               float(threshold), int(score), _ptr(mu), _ptr(var), _ptr(pr), _ptr(sc),
                                               C.byref(bv) if want_best else None, C.byref(bi) if want_best else None,
                                               self._stream())
        self._check(rc, "ppbo_predict_functionals")
        return dict(mu=mu, var=var, prob=pr, score=sc, best_val=bv.value, best_idx=bi.value)

    def marginal_axes(self, post: Posterior):
        """The ppbo_marginal_axes of a posterior: its design rows in unit-box caller coordinates (the rows themselves; an ARD
        model's scaled rows divided by the scale again, kept on the posterior; the caller's six-column rows of a camphor model with
        per-coordinate length scales) and marginal_axis_params' host arrays.  ValueError for a kernel that is not a
        product over coordinates, before anything reaches the device."""
        D = 6 if post.camphor is not None else post.X.shape[1]
        l, periodic, I0 = marginal_axis_params(post.kernel, post.theta, D, post.scale, post.camphor)
        if post.camphor is not None:
            if post.Xc is None:
                raise ValueError("predict_marginals: a camphor model without its rows in the caller's coordinates")
            Xu = post.Xc
        elif post.scale is not None:
            # once per posterior, as Gt is (the scaled rows divided by the scale again: within an ulp of the caller's)
            if post.Xu is None or post.Xu.device != post.X.device:
                post.Xu = self.scale_points(post.X, 1.0 / np.asarray(post.scale, dtype=float))
            Xu = post.Xu
        else:
            Xu = post.X
        ax = _lib.marginal_axes(Xu.data_ptr(), l, periodic, I0)
        ax._Xu = Xu
        return ax

    def predict_marginals(self, post: Posterior, dims, t, effect=EFFECT_CENTRED, kind=PAIR_PROB, want_best=True,
                          want_mu=True, want_var=True, want_prob=True, want_score=False, axes=None):
        """Main effects and interactions (ppbo_predict_marginals): row i keeps the axes dims[i] (0-based, -1 = unused; [M, 2],
        or one-dimensional [M] = one axis per row) at the values t[i] in the unit box and averages f over every other coordinate.  effect:
        EFFECT_RAW the marginal itself, EFFECT_CENTRED (default) minus the overall mean, EFFECT_INTERACTION the pure
        interaction f_de - f_d - f_e + fbar.  Returns device tensors mu / var / prob / score (None where not asked for;
        prob = P(L f > 0)) and best_val / best_idx of the quantity `kind` names (PAIR_MEAN / PAIR_VARIANCE / PAIR_PROB).
        ValueError, before anything reaches the device, for a kernel that is not a product over coordinates (RQ, Matern)
        and for rows that break the rules (marginal_rows).  Rows that already live on the device -- dims an int32 and t a
        float64 tensor of shape [M, 2] there -- are handed over as they are (the library looks at them itself), and
        axes = marginal_axes(post) may be formed once and passed to every call: such a call touches no host memory and
        can be captured into a graph."""
        effect = EFFECTS.get(effect, effect)
        if effect not in (EFFECT_RAW, EFFECT_CENTRED, EFFECT_INTERACTION):
            raise ValueError(f"predict_marginals: unknown effect {effect}")
        if kind not in (PAIR_MEAN, PAIR_VARIANCE, PAIR_PROB):
            raise ValueError(f"predict_marginals: unknown score kind {kind}")
        ax = self.marginal_axes(post) if axes is None else axes
        on_device = all(isinstance(a, torch.Tensor) and a.device == self.device and a.dim() == 2 and a.shape[1] == 2
                        and a.is_contiguous() for a in (dims, t))
        if on_device and dims.dtype == torch.int32 and t.dtype == torch.float64 and dims.shape == t.shape:
            d_dims, d_t = dims, t
        else:
            if isinstance(dims, torch.Tensor):
                dims = dims.cpu().numpy()
            if isinstance(t, torch.Tensor):
                t = t.cpu().numpy()
            dims, t = marginal_rows(dims, t, ax.Dc, effect)
            d_dims, d_t = self.dev(dims, dtype=torch.int32), self.dev(t)
        M = d_dims.shape[0]
        with_var = want_var or want_prob or kind != PAIR_MEAN
        md = self._model(post, with_var)
        mu = self.empty(M) if want_mu else None
        var = self.empty(M) if want_var else None
        pr = self.empty(M) if want_prob else None
        sc = self.empty(M) if want_score else None
        bv, bi = C.c_double(0.0), C.c_int64(-1)
        rc = self.lib.ppbo_predict_marginals(self.ctx, C.byref(md), C.byref(ax), _ptr(d_dims), _ptr(d_t), M, int(effect),
                                             int(kind), _ptr(mu), _ptr(var), _ptr(pr), _ptr(sc),
                                             C.byref(bv) if want_best else None, C.byref(bi) if want_best else None,
                                             self._stream())
        self._check(rc, "ppbo_predict_marginals")
        return dict(mu=mu, var=var, prob=pr, score=sc, best_val=bv.value, best_idx=bi.value)

    @staticmethod
    def _tournament_shapes(post: Posterior, Xa, Xb):
        """The refusals of predict_tournament that shapes alone decide (before anything reaches the device): (Ma, Mb)."""
        sa, sb = tuple(np.shape(Xa)), tuple(np.shape(Xb))
        D = 6 if post.camphor is not None else post.X.shape[1]
        if len(sa) != 2 or len(sb) != 2:
            raise ValueError(f"predict_tournament: the two sets have shapes {sa} and {sb}; [Ma, D] and [Mb, D] are required")
        if sa[1] != D or sb[1] != D:
            raise ValueError(f"predict_tournament: points of widths {sa[1]} and {sb[1]} for a model of {D} dimensions")
        if sa[0] < 1 or sb[0] < 1:
            raise ValueError("predict_tournament: an empty set")
        if sb[0] > TOURNAMENT_MAX_B:
            raise ValueError(f"predict_tournament: {sb[0]} opponents; at most {TOURNAMENT_MAX_B} per call (chunk the field)")
        return sa[0], sb[0]

    def predict_tournament(self, post: Posterior, Xa, Xb, score=TOURNAMENT_BORDA, want_cov=False, want_prob=False,
                           want_best=True):
        """Tournaments (ppbo_predict_tournament): every candidate Xa[i] against every opponent Xb[j], points in the
        caller's coordinates.  Returns device tensors mu_a / var_a [Ma] and mu_b / var_b [Mb] (bit for bit predict's),
        cov / prob [Ma, Mb] (None unless asked for: nothing of that size is formed otherwise; prob[i, j] = P(a_i > b_j)),
        score [Ma] (TOURNAMENT_BORDA: the mean of row i of prob, TOURNAMENT_WORST: its minimum) and best_val / best_idx,
        the largest score and its first row.  A non-finite opponent poisons every score.  ValueError, before anything
        reaches the device, for shape errors and more than TOURNAMENT_MAX_B opponents."""
        Ma, Mb = self._tournament_shapes(post, Xa, Xb)
        if score not in (TOURNAMENT_BORDA, TOURNAMENT_WORST):
            raise ValueError(f"predict_tournament: unknown score kind {score}")
        Xa, Xb = self._points(post, Xa), self._points(post, Xb)
        md = self._model(post, True)
        mu_a, var_a, mu_b, var_b = self.empty(Ma), self.empty(Ma), self.empty(Mb), self.empty(Mb)
        cov = self.empty(Ma, Mb) if want_cov else None
        pr = self.empty(Ma, Mb) if want_prob else None
        sc = self.empty(Ma)
        bv, bi = C.c_double(0.0), C.c_int64(-1)
        rc = self.lib.ppbo_predict_tournament(self.ctx, C.byref(md), _ptr(Xa), Ma, _ptr(Xb), Mb, int(score), _ptr(mu_a),
                                              _ptr(var_a), _ptr(mu_b), _ptr(var_b), _ptr(cov), _ptr(pr), _ptr(sc),
                                              C.byref(bv) if want_best else None, C.byref(bi) if want_best else None,
                                              self._stream())
        self._check(rc, "ppbo_predict_tournament")
        return dict(mu_a=mu_a, var_a=var_a, mu_b=mu_b, var_b=var_b, cov=cov, prob=pr, score=sc, best_val=bv.value,
                    best_idx=bi.value)

    def search_batch(self, post: Posterior, Xc, q, score=SCORE_POINTWISE_EI, mustar=0.0, noise_var=None,
                     want_var_cond=False):
        """A shortlist (ppbo_search_batch): q rows of Xc [M, D] (the caller's coordinates) picked greedily, each pick
        the first row of the largest score -- SCORE_POINTWISE_EI or SCORE_VARIANCE, with mustar as in predict -- under
        the variance CONDITIONED on the earlier picks observed with noise noise_var (None: theta[0]^2, the model's own
        noise; 0: exact observations; the mean does not change).  Returns idx [q] int64 and score [q] (NumPy; the score
        of a pick at its turn; (-1, NaN) once nothing scoreable is left), the device tensors mu, var [M] (bit for bit
        predict's) and var_cond [M], the variance after all q picks (None unless want_var_cond).  ValueError, before
        anything reaches the device, for shape errors, q outside 1 .. BATCH_MAX_Q, SCORE_MEAN or an unknown score kind,
        and a negative or non-finite noise_var."""
        shape = tuple(np.shape(Xc))
        D = 6 if post.camphor is not None else post.X.shape[1]
        if len(shape) != 2 or shape[1] != D or shape[0] < 1:
            raise ValueError(f"search_batch: candidates of shape {shape}; [M, {D}] with M >= 1 is required")
        if isinstance(q, bool) or not isinstance(q, (int, np.integer)) or not 1 <= q <= BATCH_MAX_Q:
            raise ValueError(f"search_batch: q = {q!r}; an integer in 1 .. {BATCH_MAX_Q} is required")
        if score not in (SCORE_POINTWISE_EI, SCORE_VARIANCE):
            raise ValueError(f"search_batch: score kind {score!r}; SCORE_POINTWISE_EI or SCORE_VARIANCE is required (the mean "
                             "does not change under the conditioning)")
        nv = float(post.theta[0]) ** 2 if noise_var is None else float(noise_var)
        if not (np.isfinite(nv) and nv >= 0.0):
            raise ValueError(f"search_batch: noise_var = {noise_var!r}; a finite value >= 0 is required")
        Xc = self._points(post, Xc)
        M = Xc.shape[0]
        md = self._model(post, True)
        mu, var = self.empty(M), self.empty(M)
        vc = self.empty(M) if want_var_cond else None
        idx, sc = (C.c_int64 * int(q))(), (C.c_double * int(q))()
        rc = self.lib.ppbo_search_batch(self.ctx, C.byref(md), _ptr(Xc), M, int(score), float(mustar), nv, int(q), idx, sc,
                                        _ptr(mu), _ptr(var), _ptr(vc), self._stream())
        self._check(rc, "ppbo_search_batch")
        return dict(idx=np.array(idx[:], dtype=np.int64), score=np.array(sc[:], dtype=np.float64), mu=mu, var=var,
                    var_cond=vc)

    def predict_kg(self, post: Posterior, Xa, Xb, noise_var=None, want_kinks=False, want_best=True):
        """The knowledge gradient (ppbo_predict_kg) of every candidate Xa[i] over the field Xb [Mb <= KG_MAX_B, D], points
        in the caller's coordinates: kg[i] = E[max of the mean over the field and Xa[i] after observing f(Xa[i]) with
        noise noise_var] - the same maximum now (None: theta[0]^2, the model's own noise; 0: an exact observation; the
        shortlist's convention for an imagined observation, not a preference answer).  The field should hold the current
        recommendation.  Returns device tensors kg [Ma], kinks [Ma] (int32, the kinks of each envelope; None unless
        asked for), mu_a / var_a [Ma] and mu_b / var_b [Mb] (bit for bit predict's) and best_val / best_idx, the largest
        KG and its first row.  A non-finite field point poisons every row.  ValueError, before anything reaches the
        device, for predict_tournament's shape errors and a negative or non-finite noise_var."""
        Ma, Mb = self._tournament_shapes(post, Xa, Xb)
        nv = float(post.theta[0]) ** 2 if noise_var is None else float(noise_var)
        if not (np.isfinite(nv) and nv >= 0.0):
            raise ValueError(f"predict_kg: noise_var = {noise_var!r}; a finite value >= 0 is required")
        Xa, Xb = self._points(post, Xa), self._points(post, Xb)
        md = self._model(post, True)
        kg, mu_a, var_a, mu_b, var_b = self.empty(Ma), self.empty(Ma), self.empty(Ma), self.empty(Mb), self.empty(Mb)
        kinks = torch.empty(Ma, dtype=torch.int32, device=self.device) if want_kinks else None
        bv, bi = C.c_double(0.0), C.c_int64(-1)
        rc = self.lib.ppbo_predict_kg(self.ctx, C.byref(md), _ptr(Xa), Ma, _ptr(Xb), Mb, nv, _ptr(kg), _ptr(kinks), _ptr(mu_a),
                                      _ptr(var_a), _ptr(mu_b), _ptr(var_b), C.byref(bv) if want_best else None,
                                      C.byref(bi) if want_best else None, self._stream())
        self._check(rc, "ppbo_predict_kg")
        return dict(kg=kg, kinks=kinks, mu_a=mu_a, var_a=var_a, mu_b=mu_b, var_b=var_b, best_val=bv.value, best_idx=bi.value)

    def kg_envelope(self, a, slopes, self_a=None, self_b=None):
        """E[max_j (a_j + b_ij Z)] - max_j a_j, Z ~ N(0, 1), per row i of lines (ppbo_kg_envelope): a [Mb <= KG_MAX_B] the
        intercepts shared by all rows, slopes [Ma, Mb], and optionally one more line per row, (self_a[i], self_b[i]).
        Returns device tensors kg [Ma] and kinks [Ma] (int32) and best_val / best_idx.  A row's result depends on the set
        of its lines only.  ValueError, before anything reaches the device, for shape errors."""
        sa, ss = tuple(np.shape(a)), tuple(np.shape(slopes))
        if len(sa) != 1 or len(ss) != 2 or ss[1] != sa[0] or ss[0] < 1 or not 1 <= sa[0] <= KG_MAX_B:
            raise ValueError(f"kg_envelope: intercepts of shape {sa} and slopes of shape {ss}; [Mb] and [Ma, Mb] with Ma >= 1 "
                             f"and 1 <= Mb <= {KG_MAX_B} are required")
        if (self_a is None) != (self_b is None):
            raise ValueError("kg_envelope: the own line needs both self_a and self_b")
        if self_a is not None and (tuple(np.shape(self_a)) != (ss[0],) or tuple(np.shape(self_b)) != (ss[0],)):
            raise ValueError(f"kg_envelope: own lines of shapes {tuple(np.shape(self_a))} and {tuple(np.shape(self_b))}; "
                             f"[{ss[0]}] each is required")
        Ma, Mb = ss
        a, slopes = self.dev(a), self.dev(slopes)
        self_a, self_b = (None, None) if self_a is None else (self.dev(self_a), self.dev(self_b))
        kg = self.empty(Ma)
        kinks = torch.empty(Ma, dtype=torch.int32, device=self.device)
        bv, bi = C.c_double(0.0), C.c_int64(-1)
        rc = self.lib.ppbo_kg_envelope(self.ctx, _ptr(a), _ptr(slopes), Mb, _ptr(self_a), _ptr(self_b), Ma, Mb, _ptr(kg),
                                       _ptr(kinks), C.byref(bv), C.byref(bi), self._stream())
        self._check(rc, "ppbo_kg_envelope")
        return dict(kg=kg, kinks=kinks, best_val=bv.value, best_idx=bi.value)

    def predict_cov(self, post: Posterior, Xc, shrink=SHRINKAGE):
        Xc = self._points(post, Xc)
        M = Xc.shape[0]
        md = self._model(post, True)
        mu, cov = self.empty(M), self.empty(M, M)
        rc = self.lib.ppbo_predict_cov(self.ctx, C.byref(md), _ptr(Xc), M, float(shrink), _ptr(mu), _ptr(cov),
                                       self._stream())
        self._check(rc, "ppbo_predict_cov")
        return mu, cov

    def mean_grad(self, post: Posterior, Xc):
        """mu[M] and d mu / d x [M,D] at the rows of Xc, in the caller's coordinates (ppbo_mean_grad reads the model's
        coordinate map).  ARD: d mu / d x_d = s_d d mu / d x~_d; camphor_copper_ard_kernel: through the embedding's
        Jacobian."""
        Xc = self.dev(Xc)
        if post.embedded:
            Dm = post.X.shape[1] if post.camphor is None else 6
            if Xc.dim() != 2 or Xc.shape[1] != Dm:
                raise ValueError(f"points of shape {tuple(Xc.shape)} for a model of {Dm} dimensions")
        M, D = Xc.shape
        md = self._model(post, False)
        mu, grad = self.empty(M), self.empty(M, D)
        rc = self.lib.ppbo_mean_grad(self.ctx, C.byref(md), _ptr(Xc), M, _ptr(mu), _ptr(grad), self._stream())
        self._check(rc, "ppbo_mean_grad")
        return mu, grad

    def mean_search(self, post: Posterior, cand, K=32, sep=0.05, iters=100, tol=1e-9, sync=True):
        """Device-resident maximiser of the posterior mean over the rows of `cand` (ppbo_mean_search): returns the
        refined maxima x[found, D], mu[found] as NumPy arrays.  sync=False only enqueues (h_found = NULL: nothing
        synchronises) and returns the device tensors x[K, D], mu[K] -- rows that found no start carry mu = -inf -- so
        that several searches can be queued behind each other and read back together.  Not for an ARD posterior
        (mean_search_multi is), nor for a camphor_copper_ard_kernel posterior."""
        if post.embedded:
            raise ValueError("mean_search has no per-dimension length-scale form: use mean_search_multi")
        cand = self.dev(cand)
        M, D = cand.shape
        md = self._model(post, False)
        xs, mus = self.empty(K, D), self.empty(K)
        found = C.c_int(0)
        rc = self.lib.ppbo_mean_search(self.ctx, C.byref(md), _ptr(cand), M, int(K), float(sep), int(iters), float(tol),
                                       _ptr(xs), _ptr(mus), C.byref(found) if sync else None, self._stream())
        self._check(rc, "ppbo_mean_search")
        if not sync:
            return xs, mus
        n = found.value
        return xs[:n].cpu().numpy(), mus[:n].cpu().numpy()

    def mean_search_multi(self, post: Posterior, pool, shifts, extra=None, xprev=None, K=32, sep=0.05, iters=100, tol=1e-9,
                          screen_fp32=True):
        """All trials of one mu_star call in one enqueue (ppbo_mean_search_multi): trial t searches frac(pool + shifts[t]);
        trial 0 also the rows of `extra` ("design": the posterior's own design points, nothing is copied) and the point
        `xprev`.  Returns the device tensors x[T, K, D], mu[T, K] (mu = -inf where a trial found fewer than K starts);
        nothing synchronises."""
        pool = self.dev(pool)
        M, D = pool.shape
        Dm = post.X.shape[1] if post.camphor is None else 6       # camphor: the search is in the caller's 6 coordinates
        if D != Dm:
            # the library strides pool, shifts and extra by the MODEL's D: a mismatch would read out of bounds on the device
            raise ValueError(f"mean_search_multi: pool has {D} columns, the model {Dm}")
        sh = np.ascontiguousarray(np.atleast_2d(np.asarray(shifts, dtype=np.float64)))
        T = sh.shape[0]
        if sh.shape[1] != D:
            raise ValueError("mean_search_multi: shifts must be [T, D]")
        E, ex_ptr = 0, None
        if isinstance(extra, str):
            if extra != "design":
                raise ValueError("mean_search_multi: extra is an array of points or the string 'design'")
            E = post.X.shape[0]
        elif extra is not None:
            extra = self.dev(extra)
            if extra.dim() != 2 or extra.shape[1] != D:
                raise ValueError("mean_search_multi: extra must be [E, D]")
            E, ex_ptr = extra.shape[0], extra
        xp = None
        if xprev is not None:
            xp = np.ascontiguousarray(np.asarray(xprev, dtype=np.float64).reshape(-1))
            if xp.size != D:
                raise ValueError("mean_search_multi: xprev must have D entries")
        md = self._model(post, False)
        xs, mus = self.empty(T, K, D), self.empty(T, K)
        dp = C.POINTER(C.c_double)
        # under the model's coordinate map everything is in the caller's coordinates; "design" = the model's rows there
        # (ARD: taken back to them; camphor: the caller's rows kept in post.Xc)
        rc = self.lib.ppbo_mean_search_multi(self.ctx, C.byref(md), _ptr(pool), M, sh.ctypes.data_as(dp), T, _ptr(ex_ptr), E,
                                             xp.ctypes.data_as(dp) if xp is not None else None, int(K), float(sep),
                                             int(iters), float(tol), int(bool(screen_fp32)), _ptr(xs), _ptr(mus),
                                             self._stream())
        self._check(rc, "ppbo_mean_search_multi")
        return xs, mus

    def mean_ascent(self, post: Posterior, starts, iters=100, tol=1e-9):
        starts = self.dev(starts)
        K, D = starts.shape
        md = self._model(post, False)
        xs, mus = self.empty(K, D), self.empty(K)
        its = torch.zeros(K, dtype=torch.int32, device=self.device)
        if post.camphor is not None and D != 6:
            raise ValueError(f"mean_ascent: starts of shape {tuple(starts.shape)} for a model of 6 dimensions")
        # starts, box and results in the caller's coordinates (the model's coordinate map)
        rc = self.lib.ppbo_mean_ascent(self.ctx, C.byref(md), _ptr(starts), K, int(iters), float(tol), _ptr(xs), _ptr(mus),
                                       _ptr(its), self._stream())
        self._check(rc, "ppbo_mean_ascent")
        return xs, mus, its

    def _boxes(self, boxes, D, what):
        """Host boxes [B, 2, D] (lo row, hi row) as a contiguous float64 array; the library validates the values."""
        bx = np.ascontiguousarray(np.asarray(boxes, dtype=np.float64))
        if bx.ndim == 2:
            bx = bx[None]
        if bx.ndim != 3 or bx.shape[1] != 2 or bx.shape[2] != D:
            raise ValueError(f"{what}: boxes must be [B, 2, {D}] (lo, hi), got {tuple(bx.shape)}")
        return bx

    def mean_ascent_boxes(self, post: Posterior, starts, boxes, per_box=1, iters=100, tol=1e-9):
        """mean_ascent inside boxes (ppbo_mean_ascent_boxes): start k climbs inside boxes[k // per_box], boxes [B, 2, D]
        with B = ceil(K / per_box), in the caller's coordinates.  lo == hi fixes a coordinate.  Returns the device tensors
        x[K, D], mu[K], iterations[K]; the unit box gives mean_ascent's bits."""
        starts = self.dev(starts)
        K, D = starts.shape
        Dm = post.X.shape[1] if post.camphor is None else 6
        if D != Dm:
            raise ValueError(f"mean_ascent_boxes: starts have {D} columns, the model {Dm}")
        bx = self._boxes(boxes, D, "mean_ascent_boxes")
        md = self._model(post, False)
        xs, mus = self.empty(K, D), self.empty(K)
        its = torch.zeros(K, dtype=torch.int32, device=self.device)
        rc = self.lib.ppbo_mean_ascent_boxes(self.ctx, C.byref(md), _ptr(starts), K, bx.ctypes.data_as(C.POINTER(C.c_double)),
                                             bx.shape[0], int(per_box), int(iters), float(tol), _ptr(xs), _ptr(mus),
                                             _ptr(its), self._stream())
        self._check(rc, "ppbo_mean_ascent_boxes")
        return xs, mus, its

    def mean_search_boxes(self, post: Posterior, pool, boxes, shifts=None, seeds=None, K=32, sep=0.05, iters=100, tol=1e-9,
                          screen_fp32=True):
        """T searches of the posterior mean, trial t inside boxes[t] ([T, 2, D]: lo, hi; lo == hi fixes a coordinate), in
        one enqueue (ppbo_mean_search_boxes).  The candidates of trial t are lo + (hi - lo) * frac(pool + shifts[t])
        (shifts None: the pool itself) followed by seeds[t] ([T, S, D], clipped into the box).  Returns the device tensors
        x[T, K, D], mu[T, K] (mu = -inf behind a trial's count) and count[T]; nothing synchronises."""
        pool = self.dev(pool)
        M, D = pool.shape
        Dm = post.X.shape[1] if post.camphor is None else 6       # camphor: the search is in the caller's 6 coordinates
        if D != Dm:
            # the library strides pool, boxes, shifts and seeds by the MODEL's D: a mismatch would read out of bounds
            raise ValueError(f"mean_search_boxes: pool has {D} columns, the model {Dm}")
        bx = self._boxes(boxes, D, "mean_search_boxes")
        T = bx.shape[0]
        dp = C.POINTER(C.c_double)
        sh = None
        if shifts is not None:
            sh = np.ascontiguousarray(np.atleast_2d(np.asarray(shifts, dtype=np.float64)))
            if sh.shape != (T, D):
                raise ValueError(f"mean_search_boxes: shifts must be [{T}, {D}]")
        S, sd = 0, None
        if seeds is not None:
            sd = self.dev(seeds)
            if sd.dim() != 3 or sd.shape[0] != T or sd.shape[2] != D:
                raise ValueError(f"mean_search_boxes: seeds must be [{T}, S, {D}]")
            sd = sd.contiguous()
            S = sd.shape[1]
            if S == 0:
                sd = None
        md = self._model(post, False)
        xs, mus = self.empty(T, K, D), self.empty(T, K)
        cnt = torch.zeros(T, dtype=torch.int32, device=self.device)
        rc = self.lib.ppbo_mean_search_boxes(self.ctx, C.byref(md), _ptr(pool), M, sh.ctypes.data_as(dp) if sh is not None else None,
                                             bx.ctypes.data_as(dp), T, _ptr(sd), S, int(K), float(sep), int(iters), float(tol),
                                             int(bool(screen_fp32)), _ptr(xs), _ptr(mus), _ptr(cnt), self._stream())
        self._check(rc, "ppbo_mean_search_boxes")
        return xs, mus, cnt

    ACQ_MAX_K = 1024   # starts per ppbo_acq_ascent call

    def _acq_args(self, what, post: Posterior, X, score):
        """The refusals of acq_grad / acq_ascent that need no device: (points in the model's coordinates, scale or None)."""
        if post.camphor is not None:
            raise ValueError(f"{what}: no form for camphor_copper_ard_kernel (a box in x is not a box in the embedding)")
        if score not in (SCORE_MEAN, SCORE_POINTWISE_EI, SCORE_VARIANCE):
            raise ValueError(f"{what}: unknown score kind {score!r}")
        shape = tuple(np.shape(X))
        D = post.X.shape[1]
        if len(shape) != 2 or shape[1] != D or shape[0] < 1:
            raise ValueError(f"{what}: points of shape {shape}; [M, {D}] with M >= 1 is required")
        return self._points(post, X), post.scale

    def acq_grad(self, post: Posterior, X, score=SCORE_POINTWISE_EI, mustar=0.0, want_values=True, want_grad_mu=True,
                 want_grad_var=True, want_grad_score=True):
        """Values and gradients of the acquisition at the rows of X [M, D], in the caller's coordinates (ppbo_acq_grad):
        device tensors mu, var, score [M] (None unless want_values) and grad_mu, grad_var, grad_score [M, D] (None where
        not asked for).  score: SCORE_MEAN, SCORE_POINTWISE_EI (over mustar) or SCORE_VARIANCE.  ARD: the device works on
        s (.) x and d / d x_d = s_d d / d x~_d.  ValueError for shape errors, an unknown score kind, nothing asked for, and
        a camphor_copper_ard_kernel posterior."""
        pts, scale = self._acq_args("acq_grad", post, X, score)
        if not (want_values or want_grad_mu or want_grad_var or want_grad_score):
            raise ValueError("acq_grad: nothing asked for")
        M, D = pts.shape
        md = self._model(post, True)
        mu, var, sc = (self.empty(M), self.empty(M), self.empty(M)) if want_values else (None, None, None)
        gm, gv, gs = (self.empty(M, D) if w else None for w in (want_grad_mu, want_grad_var, want_grad_score))
        rc = self.lib.ppbo_acq_grad(self.ctx, C.byref(md), _ptr(pts), M, int(score), float(mustar), _ptr(mu), _ptr(var),
                                    _ptr(sc), _ptr(gm), _ptr(gv), _ptr(gs), self._stream())
        self._check(rc, "ppbo_acq_grad")
        if scale is not None:
            for g in (gm, gv, gs):
                if g is not None:
                    self.scale_points(g, scale, out=g)
        return dict(mu=mu, var=var, score=sc, grad_mu=gm, grad_var=gv, grad_score=gs)

    def acq_ascent(self, post: Posterior, starts, score=SCORE_POINTWISE_EI, mustar=0.0, lower=None, upper=None, iters=60,
                   tol=1e-9):
        """K <= ACQ_MAX_K starts [K, D] refined by the projected Barzilai-Borwein ascent on the score inside the box
        lower <= x <= upper (None: 0 and 1; lower_d == upper_d fixes a coordinate), all in the caller's coordinates
        (ppbo_acq_ascent; nothing synchronises).  Returns device tensors x [K, D], score, mu, var [K] and iters [K]
        (int32).  ARD: the device climbs in s (.) x inside [lower s, upper s] (tol is measured there) and x comes back
        divided by s."""
        pts, scale = self._acq_args("acq_ascent", post, starts, score)
        K, D = pts.shape
        if K > self.ACQ_MAX_K:
            raise ValueError(f"acq_ascent: {K} starts; at most {self.ACQ_MAX_K} per call")
        lo = np.zeros(D) if lower is None else np.asarray(lower, dtype=np.float64).reshape(-1)
        hi = np.ones(D) if upper is None else np.asarray(upper, dtype=np.float64).reshape(-1)
        if lo.size != D or hi.size != D:
            raise ValueError(f"acq_ascent: bounds of {lo.size} and {hi.size} entries for a model of {D} dimensions")
        box = np.ascontiguousarray(np.stack([lo, hi]) * (1.0 if scale is None else scale))
        md = self._model(post, True)
        xs, sc, mu, var = self.empty(K, D), self.empty(K), self.empty(K), self.empty(K)
        its = torch.zeros(K, dtype=torch.int32, device=self.device)
        rc = self.lib.ppbo_acq_ascent(self.ctx, C.byref(md), _ptr(pts), K, self._dptr(box), int(score), float(mustar),
                                      int(iters), float(tol), _ptr(xs), _ptr(sc), _ptr(mu), _ptr(var), _ptr(its),
                                      self._stream())
        self._check(rc, "ppbo_acq_ascent")
        if scale is not None:       # back to the caller's coordinates, and into the caller's box to the last bit
            self.scale_points(xs, 1.0 / scale, out=xs)
            xs = torch.minimum(torch.maximum(xs, self.dev(lo)), self.dev(hi))
        return dict(x=xs, score=sc, mu=mu, var=var, iters=its)

    def shift_points(self, pool, shift, out=None):
        """out = frac(pool + shift) row-wise (ppbo_shift_points)."""
        pool = self.dev(pool)
        M, D = pool.shape
        out = self.empty(M, D) if out is None else out
        sh = (C.c_double * D)(*[float(v) for v in shift])
        rc = self.lib.ppbo_shift_points(self.ctx, _ptr(pool), M, D, sh, _ptr(out), self._stream())
        self._check(rc, "ppbo_shift_points")
        return out

    def line_acq(self, post: Posterior, grid, z, mustar, shrink=SHRINKAGE, jitter=0.0):
        grid = self.dev(grid)
        B, G, D = grid.shape
        if post.embedded:
            grid = self._points(post, grid.reshape(B * G, D))
            grid = grid.reshape(B, G, grid.shape[1])
        return self._line_acq(post, grid, self.dev(z), mustar, shrink, jitter)

    def _line_acq(self, post, grid, z, mustar, shrink, jitter):
        """ppbo_line_acq on a device grid [B, G, D'] that is already in the rows' coordinates."""
        B, G = grid.shape[:2]
        md = self._model(post, True)
        ei, vm = self.empty(B), self.empty(B)
        rc = self.lib.ppbo_line_acq(self.ctx, C.byref(md), _ptr(grid), B, G, float(shrink), _ptr(z), z.shape[0],
                                    float(mustar), float(jitter), _ptr(ei), _ptr(vm), self._stream())
        self._check(rc, "ppbo_line_acq")
        return ei, vm

    def line_acq_xi(self, post: Posterior, xis, xs, alphas, z, mustar, shrink=SHRINKAGE, jitter=0.0):
        """EI and varmax of the B lines {alpha * xis[b] + xs[b]} (ppbo_line_acq_xi): the grid points are formed on the
        device.  alphas: [G] (shared by all lines) or [B, G].  ARD: the line is linear in (xi, x), so s (.) xi and s (.) x
        give the scaled points at the same alpha.  camphor_copper_ard_kernel: the line is not linear in the embedding, so
        its embedded grid is formed in the caller's coordinates (ppbo_camphor_line_points) and scored by ppbo_line_acq."""
        xis, xs, alphas, z = self.dev(xis), self.dev(xs), self.dev(alphas), self.dev(z)
        B, D = xis.shape
        if xs.shape != (B, D):
            raise ValueError("line_acq_xi: xis and xs must both be [B, D]")
        per_line = alphas.dim() == 2
        G = alphas.shape[-1]
        if per_line and alphas.shape[0] != B:
            raise ValueError("line_acq_xi: per-line abscissae must be [B, G]")
        if post.camphor is not None:
            if D != 6:
                raise ValueError(f"line_acq_xi: lines of {D} coordinates for a model of 6")
            grid = self.empty(B, G, 11)
            l = np.ascontiguousarray(post.camphor, dtype=np.float64)
            rc = self.lib.ppbo_camphor_line_points(self.ctx, _ptr(xis), _ptr(xs), _ptr(alphas), int(per_line), B, G,
                                                   self._dptr(l), _ptr(grid), self._stream())
            self._check(rc, "ppbo_camphor_line_points")
            return self._line_acq(post, grid, z, mustar, shrink, jitter)
        xis, xs = self._points(post, xis), self._points(post, xs)
        S = z.shape[0]
        md = self._model(post, True)
        ei, vm = self.empty(B), self.empty(B)
        rc = self.lib.ppbo_line_acq_xi(self.ctx, C.byref(md), _ptr(xis), _ptr(xs), _ptr(alphas), int(per_line), B, G,
                                       float(shrink), _ptr(z), S, float(mustar), float(jitter), _ptr(ei), _ptr(vm),
                                       self._stream())
        self._check(rc, "ppbo_line_acq_xi")
        return ei, vm

    @staticmethod
    def _choice_groups(what, post: Posterior, B, G, Dp):
        """B groups of G points of width Dp, as shapes alone decide it."""
        D = 6 if post.camphor is not None else post.X.shape[1]
        if Dp != D:
            raise ValueError(f"{what}: points of width {Dp} for a model of {D} dimensions")
        if B < 1 or not 1 <= G <= 128:
            raise ValueError(f"{what}: {B} groups of {G} points (B >= 1 and 1 <= G <= 128 are required)")

    @staticmethod
    def _choice_draws(what, post: Posterior, G, z, e, noise_sd, jitter):
        """The refusals of line_choice / line_choice_xi that the draws and the two numbers decide (before anything reaches
        the device): returns (S, noise_sd) with noise_sd = theta[0] where None was given."""
        sz = tuple(np.shape(z))
        if len(sz) != 2 or sz[1] != G or sz[0] < 1:
            raise ValueError(f"{what}: draws z of shape {sz} for groups of {G} points ([S, {G}] with S >= 1 is required)")
        if noise_sd is None:
            noise_sd = float(post.theta[0])
        noise_sd, jitter = float(noise_sd), float(jitter)
        if not (np.isfinite(noise_sd) and noise_sd >= 0.0 and np.isfinite(jitter) and jitter >= 0.0):
            raise ValueError(f"{what}: noise_sd = {noise_sd} and jitter = {jitter} must be finite and >= 0")
        if e is None:
            if noise_sd > 0.0:
                raise ValueError(f"{what}: noise_sd = {noise_sd} > 0 needs the noise draws e [S, G]")
        elif tuple(np.shape(e)) != sz:
            raise ValueError(f"{what}: noise draws e of shape {tuple(np.shape(e))} beside z of shape {sz}")
        return sz[0], noise_sd

    def _choice_out(self, B, G, S, want_count, want_choice):
        prob = self.empty(B, G)
        count = torch.empty(B, G, dtype=torch.int32, device=self.device) if want_count else None
        choice = torch.empty(B, S, dtype=torch.int32, device=self.device) if want_choice else None
        return prob, count, choice

    def line_choice(self, post: Posterior, grid, z, e=None, noise_sd=None, shrink=SHRINKAGE, jitter=0.0,
                    want_count=False, want_choice=False):
        """The answer to a query (ppbo_line_choice): for B groups of G <= 128 points grid[B, G, D] in the caller's
        coordinates -- lines or arbitrary items -- the probability prob[b, g] that point g is the one picked, i.e. the
        share of the S draws u = mu + L z[s] + noise_sd e[s] whose maximum it is (ties to the lower index; -1 and no count
        for a draw without a number).  z, e: [S, G], shared by all groups; noise_sd = None: theta[0], the likelihood's
        noise; e = None with noise_sd = 0: the noise-free argmax of the posterior path.  Returns the device tensors
        dict(prob, count, choice) (count [B, G] and choice [B, S] int32, None where not asked for)."""
        sg = tuple(np.shape(grid))
        if len(sg) != 3:
            raise ValueError(f"line_choice: the points must be [B, G, D] (got {sg})")
        B, G = sg[:2]
        self._choice_groups("line_choice", post, B, G, sg[2])
        S, noise_sd = self._choice_draws("line_choice", post, G, z, e, noise_sd, jitter)
        grid = self.dev(grid)
        if post.embedded:
            grid = self._points(post, grid.reshape(B * G, grid.shape[2]))
            grid = grid.reshape(B, G, grid.shape[1])
        return self._line_choice(post, grid, self.dev(z), None if e is None else self.dev(e), noise_sd, shrink, jitter,
                                 want_count, want_choice)

    def _line_choice(self, post, grid, z, e, noise_sd, shrink, jitter, want_count, want_choice):
        """ppbo_line_choice on a device grid [B, G, D'] that is already in the rows' coordinates."""
        B, G = grid.shape[:2]
        S = z.shape[0]
        md = self._model(post, True)
        prob, count, choice = self._choice_out(B, G, S, want_count, want_choice)
        rc = self.lib.ppbo_line_choice(self.ctx, C.byref(md), _ptr(grid), B, G, float(shrink), _ptr(z), _ptr(e), S,
                                       float(noise_sd), float(jitter), _ptr(prob), _ptr(count), _ptr(choice),
                                       self._stream())
        self._check(rc, "ppbo_line_choice")
        return dict(prob=prob, count=count, choice=choice)

    def line_choice_xi(self, post: Posterior, xis, xs, alphas, z, e=None, noise_sd=None, shrink=SHRINKAGE, jitter=0.0,
                       want_count=False, want_choice=False):
        """line_choice on the B lines {alpha * xis[b] + xs[b]} (ppbo_line_choice_xi), the points formed on the device as
        line_acq_xi forms them: alphas [G] (shared) or [B, G]; ARD through the scaled (xi, x), camphor_copper_ard_kernel
        through its embedded grid (ppbo_camphor_line_points)."""
        sxi, sx, sa = tuple(np.shape(xis)), tuple(np.shape(xs)), tuple(np.shape(alphas))
        if len(sxi) != 2 or sx != sxi:
            raise ValueError(f"line_choice_xi: xis and xs must both be [B, D] (got {sxi} and {sx})")
        if len(sa) not in (1, 2) or (len(sa) == 2 and sa[0] != sxi[0]):
            raise ValueError(f"line_choice_xi: abscissae must be [G] or [B, G] (got {sa} for {sxi[0]} lines)")
        B, G = sxi[0], sa[-1]
        self._choice_groups("line_choice_xi", post, B, G, sxi[1])
        S, noise_sd = self._choice_draws("line_choice_xi", post, G, z, e, noise_sd, jitter)
        xis, xs, alphas, z = self.dev(xis), self.dev(xs), self.dev(alphas), self.dev(z)
        e = None if e is None else self.dev(e)
        per_line = alphas.dim() == 2
        if post.camphor is not None:
            grid = self.empty(B, G, 11)
            l = np.ascontiguousarray(post.camphor, dtype=np.float64)
            rc = self.lib.ppbo_camphor_line_points(self.ctx, _ptr(xis), _ptr(xs), _ptr(alphas), int(per_line), B, G,
                                                   self._dptr(l), _ptr(grid), self._stream())
            self._check(rc, "ppbo_camphor_line_points")
            return self._line_choice(post, grid, z, e, noise_sd, shrink, jitter, want_count, want_choice)
        xis, xs = self._points(post, xis), self._points(post, xs)
        md = self._model(post, True)
        prob, count, choice = self._choice_out(B, G, S, want_count, want_choice)
        rc = self.lib.ppbo_line_choice_xi(self.ctx, C.byref(md), _ptr(xis), _ptr(xs), _ptr(alphas), int(per_line), B, G,
                                          float(shrink), _ptr(z), _ptr(e), S, float(noise_sd), float(jitter), _ptr(prob),
                                          _ptr(count), _ptr(choice), self._stream())
        self._check(rc, "ppbo_line_choice_xi")
        return dict(prob=prob, count=count, choice=choice)

    # ---- scoring the answers ---------------------------------------------------------
    def _answer_draws(self, what, G, z, S, seed, jitter):
        """(z on the device or None, S) of loo_answers / score_answers: the given draws z [S, G], or S draws of the
        ppbo_randn stream of `seed` (None: a seed off the global NumPy stream), or none at all (S = 0: the closed-form
        scores only).  Refuses by shapes and values alone, before anything reaches the device."""
        jitter = float(jitter)
        if not (np.isfinite(jitter) and jitter >= 0.0):
            raise ValueError(f"{what}: jitter = {jitter} must be finite and >= 0")
        if z is not None:
            sz = tuple(np.shape(z))
            if len(sz) != 2 or sz[1] != G or sz[0] < 1:
                raise ValueError(f"{what}: draws z of shape {sz} for groups of {G} points ([S, {G}] with S >= 1 is required)")
            return self.dev(z), sz[0]
        S = int(S)
        if S < 0:
            raise ValueError(f"{what}: S = {S} draws")
        if S == 0:
            return None, 0
        if seed is None:
            from .random_fourier_sampler import draw_seed
            seed = draw_seed()
        return self.randn(seed, S, G), S

    def loo_answers(self, P, f, m, sigma, z=None, S=4096, seed=None, jitter=0.0, want_cov=False):
        """Leave-one-query-out scores of the answers behind a Laplace posterior N(f, P) (ppbo_loo_answers): for each of
        the n_q = N / (m + 1) stars the cavity -- the posterior without that query's likelihood site -- and the probability
        it gives the answer.  Returns the device tensors dict(lpd [n_q], agreement [n_q], edge [n_q, m + 1] (column 0 the
        agreement, column j the probability that the chosen point beats point j), cav_mean [N], cav_var [N], cav_cov
        [n_q, b, b] or None, info [n_q] int32: 0 fine, 1 P_II not positive definite, 2 the cavity is not -- NaN scores).
        z [S, m + 1]: the draws of the log score, shared by all stars; None: S draws of ppbo_randn's stream of `seed`; S = 0:
        the closed-form scores only (lpd None)."""
        sp, nf, m = tuple(np.shape(P)), int(np.prod(np.shape(f), dtype=np.int64)), int(m)
        if len(sp) != 2 or sp[0] != sp[1] or sp[0] != nf or nf < 1:
            raise ValueError(f"loo_answers: P of shape {sp} beside f of {nf} entries ([N, N] and [N] are required)")
        if not 1 <= m <= 127 or nf % (m + 1):
            raise ValueError(f"loo_answers: m = {m} for N = {nf} rows (1 <= m <= 127 and N a multiple of m + 1 are required)")
        sigma = float(sigma)
        if not (np.isfinite(sigma) and sigma > 0.0):
            raise ValueError(f"loo_answers: sigma = {sigma} must be finite and > 0")
        N, b = nf, m + 1
        z, S = self._answer_draws("loo_answers", b, z, S, seed, jitter)
        P, f = self.dev(P), self.dev(f).reshape(-1)
        n_q = N // b
        lpd = self.empty(n_q) if S > 0 else None
        agree, edge, cm, cv = self.empty(n_q), self.empty(n_q, b), self.empty(N), self.empty(N)
        cc = self.empty(n_q, b, b) if want_cov else None
        info = torch.empty(n_q, dtype=torch.int32, device=self.device)
        rc = self.lib.ppbo_loo_answers(self.ctx, _ptr(P), N, _ptr(f), N, m, sigma, _ptr(z), S, float(jitter), _ptr(lpd),
                                       _ptr(agree), _ptr(edge), _ptr(cm), _ptr(cv), _ptr(cc), _ptr(info), self._stream())
        self._check(rc, "ppbo_loo_answers")
        return dict(lpd=lpd, agreement=agree, edge=edge, cav_mean=cm, cav_var=cv, cav_cov=cc, info=info)

    def score_answers(self, post: Posterior, groups, z=None, S=4096, seed=None, shrink=SHRINKAGE, jitter=0.0):
        """Held-out scores of B new answers under the full posterior (ppbo_score_answers): groups [B, G, D] in the caller's
        coordinates, 2 <= G <= 128, point 0 of each group the chosen one.  Returns the device tensors dict(lpd [B] or None
        (S = 0), agreement [B], edge [B, G]) as loo_answers does; the draws as there."""
        sg = tuple(np.shape(groups))
        if len(sg) != 3:
            raise ValueError(f"score_answers: the points must be [B, G, D] (got {sg})")
        B, G = sg[:2]
        D = 6 if post.camphor is not None else post.X.shape[1]
        if sg[2] != D:
            raise ValueError(f"score_answers: points of width {sg[2]} for a model of {D} dimensions")
        if B < 1 or not 2 <= G <= 128:
            raise ValueError(f"score_answers: {B} groups of {G} points (B >= 1 and 2 <= G <= 128 are required)")
        z, S = self._answer_draws("score_answers", G, z, S, seed, jitter)
        grid = self.dev(groups)
        if post.embedded:
            grid = self._points(post, grid.reshape(B * G, grid.shape[2]))
            grid = grid.reshape(B, G, grid.shape[1])
        md = self._model(post, True)
        lpd = self.empty(B) if S > 0 else None
        agree, edge = self.empty(B), self.empty(B, G)
        rc = self.lib.ppbo_score_answers(self.ctx, C.byref(md), _ptr(grid), B, G, float(shrink), _ptr(z), S, float(jitter),
                                         _ptr(lpd), _ptr(agree), _ptr(edge), self._stream())
        self._check(rc, "ppbo_score_answers")
        return dict(lpd=lpd, agreement=agree, edge=edge)

    # ---- RFF -------------------------------------------------------------------------
    @staticmethod
    def _rff_widths(what, D, W, b, omega=None):
        """F = W.shape[0]; raises ValueError unless W is [F, D] for points of D columns and b (and omega) have F entries."""
        if W.dim() != 2 or W.shape[1] != D:
            raise ValueError(f"{what}: basis W of shape {tuple(W.shape)} for points of {D} columns ([F, {D}] required)")
        F = W.shape[0]
        if b.numel() != F:
            raise ValueError(f"{what}: b has {b.numel()} entries for {F} features")
        if omega is not None and omega.numel() != F:
            raise ValueError(f"{what}: omega has {omega.numel()} entries for {F} features")
        return F

    def rff_project(self, X, W, b, sigma_f, out=None):
        X, W, b = self.dev(X), self.dev(W), self.dev(b).reshape(-1)
        N, D = X.shape
        F = self._rff_widths("rff_project", D, W, b)
        Phi = self.empty(F, N) if out is None else out
        rc = self.lib.ppbo_rff_project(self.ctx, _ptr(X), N, D, _ptr(W), F, _ptr(b), float(sigma_f), _ptr(Phi),
                                       self._stream())
        self._check(rc, "ppbo_rff_project")
        return Phi

    def rff_score(self, Xc, W, b, sigma_f, omega, want_score=True):
        Xc, W, b, omega = self.dev(Xc), self.dev(W), self.dev(b).reshape(-1), self.dev(omega).reshape(-1)
        M, D = Xc.shape
        F = self._rff_widths("rff_score", D, W, b, omega)
        sc = self.empty(M) if want_score else None
        bv, bi = C.c_double(0.0), C.c_int64(-1)
        rc = self.lib.ppbo_rff_score(self.ctx, _ptr(Xc), M, D, _ptr(W), F, _ptr(b), float(sigma_f), _ptr(omega),
                                     _ptr(sc), C.byref(bv), C.byref(bi), self._stream())
        self._check(rc, "ppbo_rff_score")
        return sc, bv.value, bi.value

    def rff_omega_map(self, Phi, omega0, m, sigma, maxiter=500, gtol=1e-6):
        """Device-resident maximiser of S (ppbo_rff_omega_map): returns (omega_MAP as NumPy, S, |grad S|, iterations)."""
        Phi = self.dev(Phi)
        om = self.dev(omega0).reshape(-1).clone()
        F, N = Phi.shape
        S, gn, it = C.c_double(0.0), C.c_double(0.0), C.c_int(0)
        rc = self.lib.ppbo_rff_omega_map(self.ctx, _ptr(Phi), F, N, int(m), float(sigma), _ptr(om), int(maxiter), float(gtol),
                                         C.byref(S), C.byref(gn), C.byref(it), self._stream())
        self._check(rc, "ppbo_rff_omega_map")
        return om.cpu().numpy(), S.value, gn.value, it.value

    def randn(self, seed, *shape):
        """Standard normal draws generated on the device (ppbo_randn): a pure function of (seed, index)."""
        out = self.empty(*shape)
        rc = self.lib.ppbo_randn(self.ctx, int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(out), out.numel(), self._stream())
        self._check(rc, "ppbo_randn")
        return out

    @staticmethod
    def _camphor_coords(what, ls):
        """The `coords` argument of an RFF search: None (the identity) or the camphor map of the six length scales ls."""
        if ls is None:
            return None
        l = np.ascontiguousarray(ls, dtype=np.float64).reshape(-1)
        if l.size != 6:
            raise ValueError(f"{what}: {l.size} length scales, 6 required")
        return _lib.coords(_lib.COORDS_CAMPHOR, l)

    def _rff_search(self, what, cand, ls, W, b, sigma_f, omega, K, sep, iters, tol):
        cand, W, b, omega = self.dev(cand), self.dev(W), self.dev(b).reshape(-1), self.dev(omega).reshape(-1)
        if ls is None:
            M, D = cand.shape
        else:
            if cand.dim() != 2 or cand.shape[1] != 6:
                raise ValueError(f"{what}: candidates of shape {tuple(cand.shape)}, [M, 6] required")
            M, D = cand.shape[0], 6
        F = self._rff_widths(what, D if ls is None else 11, W, b, omega)
        xs, vals = self.empty(K, D), self.empty(K)
        found = C.c_int(0)
        co = self._camphor_coords(what, ls)
        rc = self.lib.ppbo_rff_search(self.ctx, _ptr(cand), M, D, _ptr(W), F, _ptr(b), float(sigma_f), _ptr(omega), co,
                                      int(K), float(sep), int(iters), float(tol), _ptr(xs), _ptr(vals), C.byref(found),
                                      self._stream())
        self._check(rc, "ppbo_rff_search")
        n = found.value
        return xs[:n].cpu().numpy(), vals[:n].cpu().numpy()

    def rff_search(self, cand, W, b, sigma_f, omega, K=32, sep=0.05, iters=200, tol=1e-10):
        """Device-resident maximiser of phi(x)^T omega over the rows of `cand` (ppbo_rff_search): refined maxima
        x[found, D], values[found] as NumPy arrays."""
        return self._rff_search("rff_search", cand, None, W, b, sigma_f, omega, K, sep, iters, tol)

    def rff_search_camphor(self, cand, ls, W, b, sigma_f, omega, K=32, sep=0.05, iters=200, tol=1e-10):
        """rff_search for a camphor-copper basis (ppbo_rff_search with the camphor coordinate map): W [F, 11] acts on the
        embedding e(x) of the six length scales ls; cand [M, 6], the box, sep and the refined maxima x[found, 6] are in
        the caller's coordinates.  Returns x[found, 6], values[found] as NumPy arrays."""
        return self._rff_search("rff_search_camphor", cand, ls, W, b, sigma_f, omega, K, sep, iters, tol)

    # ---- batches of posterior samples (S weight vectors per call) ---------------------------
    @staticmethod
    def _rff_multi_widths(what, D, W, b, omegas, K=None):
        """(F, S) for S weight vectors omegas [S, F] (NumPy arrays or tensors: only their shapes are read, so this runs
        before anything goes to the device); raises ValueError unless W is [F, D] for points of 1..64 columns, b has F
        entries, 1 <= S <= RFF_MULTI_MAX_S and (given) 1 <= K <= 1024."""
        if not 1 <= D <= 64:
            raise ValueError(f"{what}: points of {D} columns (1..64 supported)")
        if len(W.shape) != 2 or W.shape[1] != D:
            raise ValueError(f"{what}: basis W of shape {tuple(W.shape)} for points of {D} columns ([F, {D}] required)")
        F = W.shape[0]
        if int(np.prod(b.shape)) != F:
            raise ValueError(f"{what}: b has {int(np.prod(b.shape))} entries for {F} features")
        if len(omegas.shape) != 2 or omegas.shape[1] != F:
            raise ValueError(f"{what}: omegas of shape {tuple(omegas.shape)}, [S, {F}] required")
        S = omegas.shape[0]
        if not 1 <= S <= RFF_MULTI_MAX_S:
            raise ValueError(f"{what}: {S} samples per call (1..{RFF_MULTI_MAX_S})")
        if K is not None and not 1 <= K <= 1024:
            raise ValueError(f"{what}: K = {K} starts per sample (1..1024)")
        return F, S

    def rff_omega_draws(self, seed, omega_map, cov_diag, n):
        """[n, F] draws omega_MAP + sqrt(cov_diag) z of the posterior weights on the device (ppbo_rff_omega_draws), z the
        ppbo_randn stream of `seed`: bitwise reproducible."""
        om, cov = self.dev(omega_map).reshape(-1), self.dev(cov_diag).reshape(-1)
        F = om.numel()
        if cov.numel() != F:
            raise ValueError(f"rff_omega_draws: cov_diag has {cov.numel()} entries for {F} features")
        if int(n) < 1:
            raise ValueError(f"rff_omega_draws: n = {n} draws")
        out = self.empty(int(n), F)
        rc = self.lib.ppbo_rff_omega_draws(self.ctx, int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(om), _ptr(cov), F, int(n), _ptr(out),
                                           self._stream())
        self._check(rc, "ppbo_rff_omega_draws")
        return out

    def rff_score_multi(self, Xc, W, b, sigma_f, omegas):
        """phi(x_c)^T omega_s for S weight vectors omegas [S, F] (ppbo_rff_score_multi): a [S, M] device tensor."""
        if len(Xc.shape) != 2:
            raise ValueError(f"rff_score_multi: candidates of shape {tuple(Xc.shape)}, [M, D] required")
        M, D = Xc.shape
        F, S = self._rff_multi_widths("rff_score_multi", D, W, b, omegas)
        Xc, W, b, omegas = self.dev(Xc), self.dev(W), self.dev(b).reshape(-1), self.dev(omegas)
        sc = self.empty(S, M)
        rc = self.lib.ppbo_rff_score_multi(self.ctx, _ptr(Xc), M, D, _ptr(W), F, _ptr(b), float(sigma_f), _ptr(omegas), S,
                                           _ptr(sc), self._stream())
        self._check(rc, "ppbo_rff_score_multi")
        return sc

    def _rff_search_multi(self, what, cand, D, ls, W, b, sigma_f, omegas, K, sep, iters, tol):
        if len(cand.shape) != 2 or cand.shape[1] != D:
            raise ValueError(f"{what}: candidates of shape {tuple(cand.shape)}, [M, {D}] required")
        M = cand.shape[0]
        F, S = self._rff_multi_widths(what, D if ls is None else 11, W, b, omegas, int(K))
        cand, W, b, omegas = self.dev(cand), self.dev(W), self.dev(b).reshape(-1), self.dev(omegas)
        xs, vals = self.empty(S, K, D), self.empty(S, K)
        found = torch.zeros(S, dtype=torch.int32, device=self.device)
        co = self._camphor_coords(what, ls)
        rc = self.lib.ppbo_rff_search_multi(self.ctx, _ptr(cand), M, D, _ptr(W), F, _ptr(b), float(sigma_f), _ptr(omegas), co,
                                            S, int(K), float(sep), int(iters), float(tol), _ptr(xs), _ptr(vals), _ptr(found),
                                            self._stream())
        self._check(rc, "ppbo_rff_search_multi")
        return xs.cpu().numpy(), vals.cpu().numpy(), found.cpu().numpy()

    def rff_search_multi(self, cand, W, b, sigma_f, omegas, K=32, sep=0.05, iters=200, tol=1e-10):
        """rff_search for S weight vectors omegas [S, F] over the same candidates (ppbo_rff_search_multi): returns
        x [S, K, D], values [S, K], found [S] as NumPy; sample s's refined maxima are its rows < found[s], the others
        hold -inf values."""
        D = cand.shape[1] if len(cand.shape) == 2 else 0
        return self._rff_search_multi("rff_search_multi", cand, D, None, W, b, sigma_f, omegas, K, sep, iters, tol)

    def rff_search_multi_camphor(self, cand, ls, W, b, sigma_f, omegas, K=32, sep=0.05, iters=200, tol=1e-10):
        """rff_search_multi for a camphor-copper basis (ppbo_rff_search_multi with the camphor coordinate map): W [F, 11],
        cand [M, 6] and the results x [S, K, 6] in the caller's coordinates."""
        return self._rff_search_multi("rff_search_multi_camphor", cand, 6, ls, W, b, sigma_f, omegas, K, sep, iters, tol)

    # ---- pathwise posterior samples g_s = phi^T w_s + k(., X) v_s -------------------------------------------
    @staticmethod
    def _path_widths(what, D, W, b, Wp, V, X, kernel, theta, K=None):
        """(F, S, N, scale) of S paths (W_prior [S, F], V [S, N]) over the design X [N, D]: the checks of
        _rff_multi_widths, V's shape, a radial kernel and theta[1] (lengthscales); only shapes are read, so this runs
        before anything goes to the device.  scale: 1 / l for per-dimension length scales, else None."""
        F, S = Engine._rff_multi_widths(what, D, W, b, Wp, K)
        if kernel not in RADIAL_KERNELS:
            raise ValueError(f"{what}: pathwise samples are defined for the radial kernels {RADIAL_KERNELS}, not {kernel}")
        if len(X.shape) != 2 or X.shape[1] != D or X.shape[0] < 1:
            raise ValueError(f"{what}: design of shape {tuple(X.shape)}, [N, {D}] required")
        N = X.shape[0]
        if len(V.shape) != 2 or tuple(V.shape) != (S, N):
            raise ValueError(f"{what}: V of shape {tuple(V.shape)}, [{S}, {N}] required")
        ls = lengthscales(theta, D, kernel)
        return F, S, N, None if ls is None else 1.0 / ls

    def path_score_multi(self, Xc, W, b, theta, kernel, X, Wp, V):
        """g_s(x_c) = phi(x_c)^T w_s + k(x_c, X) v_s for S paths (ppbo_path_score_multi): a [S, M] device tensor.  Xc [M, D],
        the basis W [F, D] and the design X [N, D] in the caller's coordinates, Wp [S, F], V [S, N]; per-dimension length
        scales go through the input scaling (rows times 1 / l, basis times l)."""
        if len(Xc.shape) != 2:
            raise ValueError(f"path_score_multi: candidates of shape {tuple(Xc.shape)}, [M, D] required")
        M, D = Xc.shape
        F, S, N, scale = self._path_widths("path_score_multi", D, W, b, Wp, V, X, kernel, theta)
        Xc, W, b, X, Wp, V = self.dev(Xc), self.dev(W), self.dev(b).reshape(-1), self.dev(X), self.dev(Wp), self.dev(V)
        th = theta
        if scale is not None:
            Xc, X, W = self.scale_points(Xc, scale), self.scale_points(X, scale), self.scale_points(W, 1.0 / scale)
            th = (float(theta[0]), 1.0, float(theta[2]))
        sc = self.empty(S, M)
        rc = self.lib.ppbo_path_score_multi(self.ctx, self._kid(kernel), self._theta(th), _ptr(Xc), M, D, _ptr(W), F, _ptr(b),
                                            _ptr(Wp), _ptr(X), N, _ptr(V), S, _ptr(sc), self._stream())
        self._check(rc, "ppbo_path_score_multi")
        return sc

    def path_search_multi(self, cand, W, b, theta, kernel, X, Wp, V, K=32, sep=0.05, iters=200, tol=1e-10):
        """rff_search_multi for S paths (ppbo_path_search_multi): returns x [S, K, D], values [S, K], found [S] as NumPy;
        path s's refined maxima are its rows < found[s], the others hold -inf values.  Arguments as path_score_multi."""
        if len(cand.shape) != 2:
            raise ValueError(f"path_search_multi: candidates of shape {tuple(cand.shape)}, [M, D] required")
        M, D = cand.shape
        F, S, N, scale = self._path_widths("path_search_multi", D, W, b, Wp, V, X, kernel, theta, int(K))
        cand, W, b, X, Wp, V = self.dev(cand), self.dev(W), self.dev(b).reshape(-1), self.dev(X), self.dev(Wp), self.dev(V)
        th, co = theta, None
        if scale is not None:
            X = self.scale_points(X, scale)
            th = (float(theta[0]), 1.0, float(theta[2]))
            co = _lib.coords(_lib.COORDS_SCALED, scale)      # (keeps its copy of scale alive until the call has returned)
        xs, vals = self.empty(S, K, D), self.empty(S, K)
        found = torch.zeros(S, dtype=torch.int32, device=self.device)
        rc = self.lib.ppbo_path_search_multi(self.ctx, self._kid(kernel), self._theta(th), _ptr(cand), M, D, _ptr(W), F,
                                             _ptr(b), _ptr(Wp), _ptr(X), N, _ptr(V), co, S, int(K), float(sep), int(iters),
                                             float(tol), _ptr(xs), _ptr(vals), _ptr(found), self._stream())
        self._check(rc, "ppbo_path_search_multi")
        return xs.cpu().numpy(), vals.cpu().numpy(), found.cpu().numpy()

    def rff_terms(self, Phi, omega, m, sigma):
        Phi, omega = self.dev(Phi), self.dev(omega).reshape(-1)
        F, N = Phi.shape
        g, h = self.empty(F), self.empty(F)
        S = C.c_double(0.0)
        rc = self.lib.ppbo_rff_terms(self.ctx, _ptr(Phi), F, N, m, float(sigma), _ptr(omega), C.byref(S), _ptr(g),
                                     _ptr(h), self._stream())
        self._check(rc, "ppbo_rff_terms")
        return S.value, g, h


_default = {}


def get_engine(device: int = 0) -> Engine:
    if device not in _default:
        _default[device] = Engine(device)
    return _default[device]
