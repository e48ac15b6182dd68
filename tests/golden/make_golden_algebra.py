# -*- coding: utf-8 -*-
"""Generate tests/golden/algebra_golden.npz FROM THE REFERENCE'S OWN PYTHON -- build container only:

    python tests/golden/make_golden_algebra.py

Fixtures for the term algebra (TermProduct, TermDiff, TermConvolution): every expectation is computed by the reference's
term classes and its numpy GaussianProcess where they lie (oracle/ref_shim.py registers the one compiled module they
import), plus numpy dense algebra on the reference's K as a check.  Only inputs and expected outputs are stored (DATA: a
.npz of float64 arrays) -- no reference source text.  Per case <name>:
    <name>_ar .. _dc      get_coefficients()                                   (this pins the ORDER of the product's terms)
    <name>_c _a _U _V     get_celerite_matrices(x, diag)                       (a carries the convolution's diagonal shift)
    <name>_value          get_value at the lags `lags` = {0, delta/3, delta, 1.5 delta, 0.7, 3.0}
    <name>_K              to_dense(x, diag)
    <name>_psd            get_psd(omega)
    <name>_loglik         GaussianProcess(kernel).log_likelihood(y)
and for prod_sho_real and conv_sum: <name>_mu, <name>_var = predict(y, t=xs, return_var=True) on 20 new times whose
lags to every x are >= delta.  The script asserts that every case is positive definite and that the semiseparable
matrices reproduce the dense K.
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True   # never write __pycache__ next to the reference's modules
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import ref_shim  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("ar", "cr", "ac", "bc", "cc", "dc")


def semisep_error(x, c, a, U, V, K):
    dt = np.abs(x[:, None] - x[None, :])
    Kl = np.einsum("nj,mj,nmj->nm", U, V, np.exp(-c[None, None, :] * dt[:, :, None]))
    return max(np.max(np.abs(np.tril(Kl, -1) - np.tril(K, -1))), np.max(np.abs(a - np.diag(K)))) / np.max(np.abs(K))


def main():
    ref = ref_shim.install()
    T = ref.terms
    rng = np.random.default_rng(721)
    N = 60
    x = np.cumsum(rng.uniform(0.08, 0.3, N))
    diag = rng.uniform(0.1, 0.3, N)
    y = np.sin(x) + 0.1 * rng.standard_normal(N)
    delta, big = 0.05, 0.08
    assert np.min(np.diff(x)) > big
    sho = lambda: T.SHOTerm(S0=5.0, w0=0.8, Q=3.45)
    sho2 = lambda: T.SHOTerm(sigma=1.2, rho=2.5, Q=1.7)
    over = lambda: T.SHOTerm(S0=1.2, w0=0.3, Q=0.1)
    real = lambda: T.RealTerm(a=1.3, c=0.4)
    mat = lambda: T.Matern32Term(sigma=0.5, rho=2.0)
    rot = lambda: T.RotationTerm(sigma=1.5, period=3.45, Q0=1.3, dQ=1.05, f=0.5)
    cases = {
        "prod_sho_real": (sho() * real(), 0.0),
        "prod_sho_sho": (sho() * sho2(), 0.0),
        "prod_over_mat": (over() * mat(), 0.0),
        "prod_of_sums": ((sho() + real()) * (mat() + real()), 0.0),
        "prod_rot_real": (rot() * real(), 0.0),
        "nested": ((sho() * real()) * sho2() + real(), 0.0),
        "diff_sho": (T.TermDiff(sho()), 0.0),
        "diff_mat": (T.TermDiff(mat()), 0.0),
        "diff_rot_plus": (T.TermDiff(rot()) + real(), 0.0),
        "conv_sho": (T.TermConvolution(sho(), delta), delta),
        "conv_over": (T.TermConvolution(over(), delta), delta),
        "conv_sum": (T.TermConvolution(sho() + real(), delta), delta),
        "conv_prod": (T.TermConvolution(sho() * real() + mat(), delta), delta),
        "conv_big": (T.TermConvolution(sho() + real(), big), big),
    }
    # 20 new times, every lag to every x at least delta (midpoints of the widest gaps, and points beyond both ends)
    gaps = np.argsort(np.diff(x))[::-1][:16]
    xs = np.sort(np.concatenate([0.5 * (x[gaps] + x[gaps + 1]), [x[0] - 0.7, x[0] - 0.2, x[-1] + 0.3, x[-1] + 1.1]]))
    assert xs.size == 20 and np.min(np.abs(xs[:, None] - x[None, :])) >= delta
    omega = np.array([0.0, 0.3, 0.8, 2.0, 9.0])
    out = {"x": x, "diag": diag, "y": y, "xs": xs, "omega": omega, "delta": np.array(delta), "delta_big": np.array(big)}
    for name, (kernel, dt) in cases.items():
        lags = np.array([0.0, (dt or delta) / 3, dt or delta, 1.5 * (dt or delta), 0.7, 3.0])
        for cn, v in zip(NAMES, kernel.get_coefficients()):
            out["%s_%s" % (name, cn)] = np.asarray(v, dtype=np.float64)
        c, a, U, V = kernel.get_celerite_matrices(x, diag)
        K = kernel.to_dense(x, diag)
        err = semisep_error(x, c, a, U, V, K)
        lam = np.linalg.eigvalsh(K)
        assert lam[0] > 0.05, (name, lam[0])          # positive definite with the reference alone
        assert err < 2e-13, (name, err)
        gp = ref.numpy.GaussianProcess(kernel)
        gp.compute(x, diag=diag)
        ll = float(gp.log_likelihood(y))
        L = np.linalg.cholesky(K)
        al = np.linalg.solve(L, y)
        want = -0.5 * (al @ al) - np.sum(np.log(np.diag(L))) - 0.5 * N * np.log(2 * np.pi)
        assert abs(ll - want) <= 1e-10 * abs(want), (name, ll, want)
        out[name + "_c"], out[name + "_a"], out[name + "_U"], out[name + "_V"] = c, a, U, V
        out[name + "_lags"] = lags
        out[name + "_value"] = kernel.get_value(lags)
        out[name + "_K"] = K
        out[name + "_psd"] = kernel.get_psd(omega)
        out[name + "_loglik"] = np.array(ll)
        if name in ("prod_sho_real", "conv_sum"):
            mu, var = gp.predict(y, t=xs, return_var=True)
            Ks = kernel.get_value(xs[:, None] - x[None, :])
            np.testing.assert_allclose(mu, Ks @ np.linalg.solve(K, y), rtol=1e-9, atol=1e-10)
            np.testing.assert_allclose(var, kernel.get_value(0.0) - np.einsum("mn,nm->m", Ks, np.linalg.solve(K, Ks.T)),
                                       rtol=1e-8, atol=1e-10)
            out[name + "_mu"], out[name + "_var"] = mu, var
        print("%-14s J=%2d  cond %.1e  lam_min %.3f  semisep %.1e  ll %.6f"
              % (name, c.size, lam[-1] / lam[0], lam[0], err, ll))
    path = os.path.join(HERE, "algebra_golden.npz")
    np.savez_compressed(path, **{k: np.asarray(v, dtype=np.float64) for k, v in out.items()})
    print("wrote", path, os.path.getsize(path), "bytes")
    ref_shim.uninstall()


if __name__ == "__main__":
    main()
