"""Covariance functions with the reference's call signature (src/kernels.py:19-53), evaluated
by the HIP cross-covariance kernel (ppbo_cross_cov).  Inputs/outputs are NumPy arrays; the
function objects carry the reference's __name__ because Hsampler dispatches on it
(src/random_fourier_sampler.py:27,40)."""
from __future__ import annotations

import numpy as np

from .engine import get_engine


def _eval(name, X1, X2, theta):
    # theta[1]: a scalar or, for the radial kernels, one length scale per input dimension (engine.lengthscales)
    if np.any(np.asarray(theta[1]) <= 0) or theta[2] <= 0:
        print("Check hyperparameter values!")          # the reference only prints (src/kernels.py:22-23)
    X1 = np.atleast_2d(np.asarray(X1, dtype=np.float64))
    X2 = np.atleast_2d(np.asarray(X2, dtype=np.float64))
    return get_engine().cross_cov(X1, X2, theta, name).cpu().numpy()


def SE_kernel(X1, X2, theta):
    return _eval("SE_kernel", X1, X2, theta)


def RQ_kernel(X1, X2, theta):
    return _eval("RQ_kernel", X1, X2, theta)


def camphor_copper_kernel(X1, X2, theta):
    return _eval("camphor_copper_kernel", X1, X2, theta)


# No reference counterpart: the GPy / scikit-learn Matern(nu) kernels, k = sigma_f^2 (1 + a + a^2/3) e^-a with
# a = sqrt(5) r / l (nu = 5/2) and k = sigma_f^2 (1 + a) e^-a with a = sqrt(3) r / l (nu = 3/2), theta = [sigma, l, sigma_f]
def Matern52_kernel(X1, X2, theta):
    return _eval("Matern52_kernel", X1, X2, theta)


def Matern32_kernel(X1, X2, theta):
    return _eval("Matern32_kernel", X1, X2, theta)


# No reference counterpart: camphor-copper with one length scale per coordinate (x, y, z, alpha, beta, gamma),
# theta = [sigma, l, sigma_f] with l a length-6 vector or a scalar standing for the reference's (l, l, l + 0.05, l, l, l);
# evaluated as SE on the embedded rows of engine.camphor_embed
def camphor_copper_ard_kernel(X1, X2, theta):
    return _eval("camphor_copper_ard_kernel", X1, X2, theta)


BY_NAME = {f.__name__: f for f in (SE_kernel, RQ_kernel, camphor_copper_kernel, Matern52_kernel, Matern32_kernel,
                                   camphor_copper_ard_kernel)}
