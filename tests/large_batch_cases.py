# -*- coding: utf-8 -*-
"""The table behind tests/test_gpu_large_batch.py and tests/test_large_batch_table.py: one row per public op (and per width,
right-hand-side count or method where the op dispatches on it) at B = 70000 series built from D = 7 distinct ones repeated.

70000 is no multiple of 64 (a partial last wavefront), 7 divides it, and 65535 mod 7 = 1, 65536 mod 7 = 2: a series index that
wraps at either grid limit lands on another of the seven series and shows as a mismatch.

A row holds
    build()            -> dict of numpy inputs, every array with the leading axis D (keys starting with "_": not arrays of the
                          batch -- programs, counts of things);
    ref(cpu, inp)      -> dict name -> numpy reference (D, ...) from the oracle / restatement call the op's own test file uses
                          ("flag": the oracle's own flags, (D,) int);
    run(ops, torch, T) -> dict name -> device tensor (B, ...) for T = the inputs expanded to B series; caller outputs are
                          pre-filled with NaN;
    crit[name]         -> allowed(xo, keep, inp) -> numpy array like xo: the bound of the op's existing test, evaluated on the seven;
    bits               -> None, or why every series must ALSO equal its repeat bit for bit (only where one kernel serves the
                          whole batch and the op's own tests already assert that replicas are bit-identical);
    fail               -> True: series FAIL of the seven gets a non-positive pivot; flag != 0 exactly there;
    plan               -> None, or (hook, the mapping the launcher's plan must report for the call).

Nothing here is new reference mathematics: the draws are inverse_diag_ref.draw / the *_ref.case helpers / oracle.dense, the
references the oracle and the *_ref restatements.  Test infrastructure only."""
import numpy as np

B, D = 70000, 7
REPS = B // D
FAIL = 3                      # the one of the seven that fails in a `fail` row
WIDTHS = (2, 3, 8)            # one lane per series, a group of four, the width-8 families
N, M = 4, 3                   # rows; new times


# ---- criteria: allowed(xo, keep, inp) on the seven references -------------------------------------------------------------------
def _amax(x):
    x = np.abs(x[np.isfinite(x)])
    return float(x.max()) if x.size else 0.0


def close(tol=1e-10, floor=1e-12):
    """test_gpu_ops.close / test_gpu_kron.close / test_gpu_terms.close: tol |b| + floor max(1, max |b|)."""
    return lambda xo, keep, inp=None: tol * np.abs(xo) + floor * max(1.0, _amax(xo[keep]))


def err(floor=None, zero_floor=None):
    """inverse_diag_ref.err <= 1: 1e-10 |xo| + 1e-12 floor, floor = max |xo| unless given; an all-zero reference is met
    exactly (the check() of the *_ref based files) unless `zero_floor` gives it a scale (test_gpu_filter_rev.check)."""
    def allowed(xo, keep, inp=None):
        f = _amax(xo[keep]) if floor is None else float(floor)
        if floor is None and f == 0.0 and zero_floor is not None:
            f = float(zero_floor)
        return 1e-10 * np.abs(xo) + 1e-12 * f
    return allowed


def per_series(scale):
    """an absolute bound per series, scale (D,)"""
    return lambda xo, keep, inp=None: np.broadcast_to(scale.reshape((D,) + (1,) * (xo.ndim - 1)), xo.shape).copy()


def rowmax(tol):
    """tol of each series' largest entry of the array (an all-zero row: exact up to tol)"""
    def allowed(xo, keep, inp=None):
        top = np.max(np.abs(xo.reshape(D, -1)), axis=1) if xo[0].size else np.ones(D)
        return per_series(tol * np.where(top == 0.0, 1.0, top))(xo, keep)
    return allowed


def relative(tol):
    return lambda xo, keep, inp=None: tol * np.abs(xo)


def elementwise(bound):
    """a bound given element by element (same shape as xo)"""
    return lambda xo, keep, inp=None: np.broadcast_to(bound, xo.shape).copy()


EXACT = lambda xo, keep, inp=None: np.zeros_like(xo)


def worst_ratio(torch, x, xo, allowed, keep, where_ref=False):
    """max |x - xo| / allowed over the kept series of ALL B, on the device in one expression; NaN must sit exactly where the
    reference has it (where_ref: positions the reference left NaN are not compared)."""
    xv = x.reshape((REPS, D) + tuple(x.shape[1:]))[:, keep]
    xo, allowed = xo[keep][None], allowed[keep][None]
    nan = torch.isnan(xo).expand_as(xv)
    if not where_ref:
        assert torch.equal(torch.isnan(xv), nan), "NaN where the reference has none (or a value where it has NaN)"
    diff = (xv - xo).abs()
    ratio = torch.where(diff == 0, torch.zeros_like(diff), diff / allowed.expand_as(diff))
    ratio = torch.where(nan, torch.zeros_like(ratio), ratio)
    assert not bool(torch.isnan(ratio).any()), "NaN outside the reference's NaN positions"
    return float(ratio.max()) if ratio.numel() else 0.0


def expand(torch, x):
    """(D, ...) numpy -> (B, ...) on the device: series b is draw b mod D"""
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return t.repeat((REPS,) + (1,) * (t.dim() - 1)).contiguous()


def nan_like(torch, *shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")


# ---- the table ---------------------------------------------------------------------------------------------------------------
class Row:
    def __init__(self, id, names, build, ref, run, crit, *, fail=False, bits=None, where_ref=(), symbols=None, plan=None, ragged=False):
        self.id, self.build, self.ref, self.run, self.crit = id, build, ref, run, crit
        self.ops = tuple(names)                                  # names of celerite2_amd.ops
        self.symbols = tuple("c2_" + n for n in names) if symbols is None else tuple(symbols)
        self.fail, self.bits, self.where_ref, self.plan = fail, bits, set(where_ref), plan
        self.ragged = ragged           # rows beyond a per-series count stay NaN in the reference: never written

    @property
    def keep(self):
        return [b for b in range(D) if not (self.fail and b == FAIL)]


ROWS = []


def add(*a, **kw):
    ROWS.append(Row(*a, **kw))


def _draws(seed, n, J, **kw):
    import inverse_diag_ref as IR
    return [IR.draw(1000 * seed + k, n, J, **kw) for k in range(D)]


def _stack(ds, keys):
    return {k: np.stack([d[k] for d in ds]) for k in keys}


def core_inputs(seed, J, n=N, fail=False):
    inp = _stack(_draws(seed, n, J), "tcaUVy")
    if fail:
        inp["a"][FAIL, n // 2] = -5.0        # a non-positive pivot at row n // 2 of one series
    return inp


def host_factor(cpu, inp, with_S=False):
    """(d, W[, S], flag) of the seven by the oracle; a failing series keeps what the oracle left."""
    t, c, a, U, V = (inp[k] for k in "tcaUV")
    n, J = U.shape[1:]
    d, W, S, flag = np.full((D, n), np.nan), np.full((D, n, J), np.nan), np.full((D, n, J, J), np.nan), np.zeros(D, dtype=np.int64)
    for b in range(D):
        flag[b] = cpu.factor_flag(t[b], c[b], a[b], U[b], V[b], d[b], W[b], S[b])
    return (d, W, S, flag) if with_S else (d, W, flag)


BITS_LOGLIK = "one kernel family serves the batch; test_gpu_ops.test_config2_full_batch_one_gpu asserts replicas bit-identical"
BITS_SOLVE = "nrhs < 8: the row kernel serves the batch; test_gpu_ops.test_many_rhs_at_full_size asserts replicas bit-identical"
BITS_KRON = "test_gpu_kron.test_config4_full_shape asserts replicas of the collapsed method bit-identical"


# -- factor --------------------------------------------------------------------------------------------------------------------
def _factor_row(J, with_S, fail):
    def build():
        return core_inputs(1, J, fail=fail)

    def ref(cpu, inp):
        d, W, S, flag = host_factor(cpu, inp, True)
        out = dict(d=d, W=W, flag=flag)
        if with_S:
            out["S"] = S
        return out

    def run(ops, torch, T):
        S = nan_like(torch, B, N, J, J) if with_S else None
        res = ops.factor(T["t"], T["c"], T["a"], T["U"], T["V"], d=nan_like(torch, B, N), W=nan_like(torch, B, N, J), S=S)
        return dict(zip(("d", "W", "S", "flag") if with_S else ("d", "W", "flag"), res))

    add("factor[J=%d%s%s]" % (J, ",S" if with_S else "", ",fail" if fail else ""), ["factor"], build, ref, run,
        dict(d=close(), W=close(), S=close()), fail=fail)


for _J in WIDTHS:
    _factor_row(_J, False, False)
    _factor_row(_J, True, False)
_factor_row(2, True, True)
_factor_row(8, False, True)


# -- the four sweeps, dot_tril, condition ----------------------------------------------------------------------------------
def _sweep_inputs(cpu, seed, J, nrhs):
    inp = core_inputs(seed, J)
    inp["d"], inp["W"], _ = host_factor(cpu, inp)
    rng = np.random.default_rng(seed)
    inp["Y"] = rng.standard_normal((D, N, nrhs))
    inp["bZ"] = rng.standard_normal((D, N, nrhs))
    return inp


def _sweep_fwd(cpu, name, inp):
    sec = inp["W"] if name.startswith("solve") else inp["V"]
    Z, F = np.empty_like(inp["Y"]), np.empty(inp["U"].shape + (inp["Y"].shape[-1],))
    for b in range(D):
        getattr(cpu, name + "_fwd")(inp["t"][b], inp["c"][b], inp["U"][b], sec[b], inp["Y"][b], Z[b], F[b])
    return sec, Z, F


def _sweep_row(name, J, nrhs):
    solve = name.startswith("solve")

    def build():
        from oracle import cpu
        return _sweep_inputs(cpu, 2, J, nrhs)

    def ref(cpu, inp):
        _, Z, F = _sweep_fwd(cpu, name, inp)
        return dict(Z=Z, F=F)

    def run(ops, torch, T):
        sec = T["W"] if solve else T["V"]
        kw = {} if solve else dict(zero_z=True)     # (backprop.*_fwd zero Z first: the NaN must not survive)
        Z, F = getattr(ops, name)(T["t"], T["c"], T["U"], sec, T["Y"], Z=nan_like(torch, B, N, nrhs), F=nan_like(torch, B, N, J, nrhs), **kw)
        return dict(Z=Z, F=F)

    add("%s[J=%d,nrhs=%d]" % (name, J, nrhs), [name], build, ref, run, dict(Z=close(), F=close()),
        bits=BITS_SOLVE if solve else None)

    def build_rev():   # (Z and F of the forward call are inputs of the reverse: the oracle's)
        from oracle import cpu
        inp = _sweep_inputs(cpu, 2, J, nrhs)
        _, inp["Z"], inp["F"] = _sweep_fwd(cpu, name, inp)
        return inp

    def ref_rev(cpu, inp):
        sec, Z, F = (inp["W"] if solve else inp["V"]), inp["Z"], inp["F"]
        outs = [np.empty((D, N)), np.empty((D, J)), np.empty((D, N, J)), np.empty((D, N, J)), np.empty((D, N, nrhs))]
        for b in range(D):
            getattr(cpu, name + "_rev")(inp["t"][b], inp["c"][b], inp["U"][b], sec[b], inp["Y"][b], Z[b], F[b], inp["bZ"][b],
                                        *[o[b] for o in outs])
        return dict(zip(("bt", "bc", "bU", "bW", "bY"), outs))

    def run_rev(ops, torch, T):
        sec = T["W"] if solve else T["V"]
        res = getattr(ops, name + "_rev")(T["t"], T["c"], T["U"], sec, T["Y"], T["Z"], T["F"], T["bZ"])
        return dict(zip(("bt", "bc", "bU", "bW", "bY"), res))

    # (the sweep reverses send B mod 8 series to another kernel: criterion only)
    add("%s_rev[J=%d,nrhs=%d]" % (name, J, nrhs), [name + "_rev"], build_rev, ref_rev, run_rev,
        {k: close() for k in ("bt", "bc", "bU", "bW", "bY")})


for _name in ("solve_lower", "solve_upper", "matmul_lower", "matmul_upper"):
    for _J in WIDTHS:
        for _nrhs in (1, 3):
            _sweep_row(_name, _J, _nrhs)


def _dot_tril_row(J, nrhs):
    def build():
        from oracle import cpu
        return _sweep_inputs(cpu, 3, J, nrhs)

    def ref(cpu, inp):   # test_gpu_ops.test_wide_models: z = Y sqrt(d), then the oracle's matmul_lower in place
        Z = np.empty_like(inp["Y"])
        for b in range(D):
            z = inp["Y"][b] * np.sqrt(inp["d"][b])[:, None]
            cpu.matmul_lower(inp["t"][b], inp["c"][b], inp["U"][b], inp["W"][b], z.copy(), z)
            Z[b] = z
        return dict(Z=Z)

    def run(ops, torch, T):
        return dict(Z=ops.dot_tril(T["t"], T["c"], T["U"], T["W"], T["d"], T["Y"], Z=nan_like(torch, B, N, nrhs)))

    add("dot_tril[J=%d,nrhs=%d]" % (J, nrhs), ["dot_tril"], build, ref, run, dict(Z=close()))


for _J in WIDTHS:
    _dot_tril_row(_J, 1 if _J == 3 else 3)


def _condition_row(J):
    def ref(cpu, inp):   # test_gpu_ops.test_condition_number_per_series: |kappa - max a / d| <= 1e-10 kappa
        d, _, flag = host_factor(cpu, inp)
        return dict(kappa=np.max(inp["a"] / d, axis=1), flag=flag)

    def run(ops, torch, T):
        kappa, flag = ops.condition(T["t"], T["c"], T["a"], T["U"], T["V"])
        return dict(kappa=kappa, flag=flag)

    add("condition[J=%d]" % J, ["condition"], lambda: core_inputs(4, J), ref, run, dict(kappa=relative(1e-10)))


for _J in WIDTHS:
    _condition_row(_J)


# -- prediction products --------------------------------------------------------------------------------------------------------
def _general_row(name, J, nrhs):
    """t1: N = 4 rows with U; t2: M = 3 rows with V, Y (test_gpu_ops.test_wide_models' layout, ties and both ends included)."""
    def build():
        ds = _draws(5, M, J)
        inp = {"t2": np.stack([d["t"] for d in ds]), "c": np.stack([d["c"] for d in ds]), "V": np.stack([d["V"] for d in ds])}
        rng = np.random.default_rng(55 + J)
        t2 = inp["t2"]
        inp["t1"] = np.sort(np.concatenate([t2[:, :1] - 1.0, t2[:, 1:2], t2[:, 1:2] + 0.013, t2[:, -1:] + 1.0], axis=1), axis=1)
        inp["U"] = rng.standard_normal((D, N, J))
        inp["Y"] = rng.standard_normal((D, M, nrhs))
        return inp

    def ref(cpu, inp):
        Z, F = np.zeros((D, N, nrhs)), np.full((D, M, J * nrhs), np.nan)
        for b in range(D):
            getattr(cpu, name + "_fwd")(inp["t1"][b], inp["t2"][b], inp["c"][b], inp["U"][b], inp["V"][b], inp["Y"][b], Z[b], F[b])
        return dict(Z=Z, F=F.reshape(D, M, J, nrhs))

    def run(ops, torch, T):
        Z, F = getattr(ops, name)(T["t1"], T["t2"], T["c"], T["U"], T["V"], T["Y"], Z=nan_like(torch, B, N, nrhs),
                                  F=nan_like(torch, B, M, J, nrhs), zero_z=True)
        return dict(Z=Z, F=F)

    # F: the rows the oracle wrote (test_wide_models compares `seen` only)
    add("%s[J=%d,nrhs=%d]" % (name, J, nrhs), [name], build, ref, run, dict(Z=close(), F=close()), where_ref=("F",),
        plan=("general_chunks", 0))


for _name in ("general_matmul_lower", "general_matmul_upper"):
    for _J in WIDTHS:
        _general_row(_name, _J, 3 if _J == 3 else 1)


# -- factor_rev ----------------------------------------------------------------------------------------------------------------
def _factor_rev_row(J):
    def build():
        from oracle import cpu
        inp = core_inputs(6, J)
        inp["d"], inp["W"], inp["S"], _ = host_factor(cpu, inp, True)
        rng = np.random.default_rng(6)
        inp["bd"], inp["bW"] = rng.standard_normal((D, N)), rng.standard_normal((D, N, J))
        return inp

    def ref(cpu, inp):
        outs = [np.empty((D, N)), np.empty((D, J)), np.empty((D, N)), np.empty((D, N, J)), np.empty((D, N, J))]
        for b in range(D):
            cpu.factor_rev(*[inp[k][b] for k in ("t", "c", "a", "U", "V", "d", "W", "S", "bd", "bW")], *[o[b] for o in outs])
        return dict(zip(("bt", "bc", "ba", "bU", "bV"), outs))

    def run(ops, torch, T):
        return dict(zip(("bt", "bc", "ba", "bU", "bV"), ops.factor_rev(*[T[k] for k in ("t", "c", "a", "U", "V", "d", "W", "S", "bd", "bW")])))

    add("factor_rev[J=%d]" % J, ["factor_rev"], build, ref, run, {k: close() for k in ("bt", "bc", "ba", "bU", "bV")})


for _J in WIDTHS:
    _factor_rev_row(_J)


# -- the matrices from the coefficients, their reverse, the kernel on two grids, the variance's quadratic form ---------------
def _coeffs(rng, Jr, Jc):
    from test_gpu_terms import coeffs
    return dict(zip(("ar", "cr", "ac", "bc", "cc", "dc"), coeffs(D, Jr, Jc, rng)))


def _terms_inputs(seed, Jr, Jc, fail=False):
    """test_gpu_terms.test_loglik_terms_vs_oracle_chain's draw"""
    rng = np.random.default_rng(seed)
    inp = _coeffs(rng, Jr, Jc)
    inp["x"] = np.sort(rng.uniform(0, N / 10.0, (D, N)), axis=1)
    inp["diag"] = rng.uniform(0.1, 0.3, (D, N))
    inp["y"] = np.sin(inp["x"]) + 0.1 * rng.standard_normal((D, N))
    if fail:
        inp["diag"][FAIL, N // 2] = -50.0
    return inp


def _matrices_ref(cpu, inp):
    from oracle import dense
    out = [dense.celerite_matrices(dense.Coeffs(**{k: inp[k][b] for k in ("ar", "cr", "ac", "bc", "cc", "dc")}), inp["x"][b], inp["diag"][b])
           for b in range(D)]
    return dict(a=np.stack([o[1] for o in out]), U=np.stack([o[2] for o in out]), V=np.stack([o[3] for o in out]))


add("get_celerite_matrices[Jr=1,Jc=1]", ["get_celerite_matrices"], lambda: _terms_inputs(7, 1, 1), _matrices_ref,
    lambda ops, torch, T: dict(zip("aUV", ops.get_celerite_matrices(T["ar"], T["ac"], T["bc"], T["dc"], T["x"], T["diag"]))),
    dict(a=close(1e-13), U=close(1e-12), V=close(1e-12)))     # test_gpu_ops.test_get_celerite_matrices_batched


def _chain(cpu, inp):
    from oracle import dense
    return [dense.coefficient_chain(cpu, *[inp[k][b] for k in ("ar", "cr", "ac", "bc", "cc", "dc", "x", "diag", "y")]) for b in range(D)]


TERM_GRADS = ("bar", "bcr", "bac", "bbc", "bcc", "bdc", "bx", "bdiag", "by")


def _matrices_rev_build():
    """The cotangents are the oracle's own log-likelihood gradients in (t, c, a, U, V): the expected output is then what
    oracle.dense.coefficient_chain pushes them to."""
    from oracle import cpu, dense
    inp = _terms_inputs(8, 1, 1)
    g = []
    for b in range(D):
        c, a, U, V = dense.celerite_matrices(dense.Coeffs(**{k: inp[k][b] for k in ("ar", "cr", "ac", "bc", "cc", "dc")}), inp["x"][b], inp["diag"][b])
        _, grads, flag = cpu.loglik_grad(inp["x"][b], c, a, U, V, inp["y"][b])
        assert flag == 0
        g.append((V,) + tuple(grads[:5]))
    for i, k in enumerate(("V", "bt", "bcv", "ba", "bU", "bV")):
        inp[k] = np.stack([x[i] for x in g])
    return inp


def _matrices_rev_ref(cpu, inp):
    want = _chain(cpu, inp)
    return {k: np.stack([w[1][i] for w in want]) for i, k in enumerate(TERM_GRADS[:8])}


add("get_celerite_matrices_rev[Jr=1,Jc=1]", ["get_celerite_matrices_rev"], _matrices_rev_build, _matrices_rev_ref,
    lambda ops, torch, T: dict(zip(TERM_GRADS[:8], ops.get_celerite_matrices_rev(T["ac"], T["bc"], T["dc"], T["x"], T["V"], T["bt"], T["bcv"],
                                                                                 T["ba"], T["bU"], T["bV"], 1))),
    {k: close() for k in TERM_GRADS[:8]})


def _kernel_values_row(n):
    """N = M = 8: the tiled kernel's only failing condition is B; N = M = 3: the thread-per-entry kernel either way."""
    def build():
        rng = np.random.default_rng(9 + n)
        inp = _coeffs(rng, 1, 1)
        inp["t1"], inp["t2"] = rng.uniform(0.0, 4.0, (D, n)), rng.uniform(-0.5, 4.5, (D, n))
        return inp

    def ref(cpu, inp):
        from oracle import dense
        K = np.stack([dense.kernel_value(dense.Coeffs(**{k: inp[k][b] for k in ("ar", "cr", "ac", "bc", "cc", "dc")}),
                                         inp["t1"][b][:, None] - inp["t2"][b][None, :]) for b in range(D)])
        return dict(K=K)

    def crit(xo, keep, inp):   # test_gpu_ops.test_kernel_values_factored_exponential: 2e-13 of k(0) = sum ar + sum ac per entry
        return per_series(2e-13 * (inp["ar"].sum(1) + inp["ac"].sum(1)))(xo, keep)

    add("kernel_values[N=M=%d]" % n, ["kernel_values"], build, ref,
        lambda ops, torch, T: dict(K=ops.kernel_values(*[T[k] for k in ("ar", "cr", "ac", "bc", "cc", "dc", "t1", "t2")])), dict(K=crit))


_kernel_values_row(8)
_kernel_values_row(3)


def _colsumsq_build():
    rng = np.random.default_rng(10)
    return dict(Z=rng.standard_normal((D, N, M)), d=rng.uniform(0.2, 2.0, (D, N)))


# (no test of its own besides gp.predict's; the definition in its docstring, a sum of N non-negative terms of three roundings
# each: far inside the standing 1e-10)
add("colsumsq_over_d", ["colsumsq_over_d"], _colsumsq_build,
    lambda cpu, inp: dict(out=(inp["Z"] ** 2 / inp["d"][:, :, None]).sum(axis=1)),
    lambda ops, torch, T: dict(out=ops.colsumsq_over_d(T["Z"], T["d"])), dict(out=close()))


# -- the fused log-likelihoods ------------------------------------------------------------------------------------------------
LOGLIK_GRADS = ("bt", "bc", "ba", "bU", "bV", "by")


def _loglik_ref(cpu, inp):
    ll, grads, flag = cpu.loglik_grad_batched(*[inp[k] for k in "tcaUVy"], nthreads=2)
    return dict(zip(("ll",) + LOGLIK_GRADS, (ll,) + tuple(grads)), flag=flag)


# the mapping c2_internal_loglik_grad_plan reports at 70000 x 4 by width (c2::Lanes: 1 one lane per series, 8 a group of lanes)
LOGLIK_MAPPING = {2: 1, 3: 8, 8: 1}


def _loglik_row(J, fail):
    tag = "[J=%d%s]" % (J, ",fail" if fail else "")
    add("loglik" + tag, ["loglik"], lambda: core_inputs(11, J, fail=fail), lambda cpu, inp: {k: v for k, v in _loglik_ref(cpu, inp).items() if k in ("ll", "flag")},
        lambda ops, torch, T: dict(zip(("ll", "flag"), ops.loglik(*[T[k] for k in "tcaUVy"]))), dict(ll=close()), fail=fail,
        bits=BITS_LOGLIK)

    def run(ops, torch, T):
        out = tuple(nan_like(torch, *s) for s in ((B, N), (B, J), (B, N), (B, N, J), (B, N, J), (B, N)))
        ll, grads, flag = ops.loglik_grad(*[T[k] for k in "tcaUVy"], out=out)
        return dict(zip(("ll",) + LOGLIK_GRADS, (ll,) + tuple(grads)), flag=flag)

    add("loglik_grad" + tag, ["loglik_grad"], lambda: core_inputs(11, J, fail=fail), _loglik_ref, run,
        {k: close() for k in ("ll",) + LOGLIK_GRADS}, fail=fail, bits=BITS_LOGLIK, plan=("loglik_grad", LOGLIK_MAPPING[J]))


for _J in WIDTHS:
    _loglik_row(_J, False)
_loglik_row(2, True)
_loglik_row(8, True)


# the mapping c2_internal_loglik_terms_plan reports at 70000 series by width (c2::Lanes: 1 one lane per series -- the fused kernels
# of the chip-filling batch; 13 the composed chain, for the widths without fused kernels)
TERMS_MAPPING = {2: 1, 3: 13, 8: 1}


def _terms_row(Jr, Jc, fail):
    tag = "[Jr=%d,Jc=%d%s]" % (Jr, Jc, ",fail" if fail else "")
    keys = ("ar", "cr", "ac", "bc", "cc", "dc", "x", "diag", "y")

    def ref(cpu, inp):
        want = _chain(cpu, inp)
        out = dict(ll=np.array([w[0] for w in want]), flag=np.array([w[2] for w in want]))
        out.update({k: np.stack([np.asarray(w[1][i]) for w in want]) for i, k in enumerate(TERM_GRADS)})
        return out

    add("loglik_terms" + tag, ["loglik_terms"], lambda: _terms_inputs(12, Jr, Jc, fail),
        lambda cpu, inp: {k: v for k, v in ref(cpu, inp).items() if k in ("ll", "flag")},
        lambda ops, torch, T: dict(zip(("ll", "flag"), ops.loglik_terms(*[T[k] for k in keys]))), dict(ll=close()), fail=fail,
        plan=("loglik_terms", TERMS_MAPPING[Jr + 2 * Jc]))

    def run(ops, torch, T):
        out = tuple(nan_like(torch, *s) for s in ((B, Jr), (B, Jr), (B, Jc), (B, Jc), (B, Jc), (B, Jc), (B, N), (B, N), (B, N)))
        ll, grads, flag = ops.loglik_terms_grad(*[T[k] for k in keys], out=out)
        return dict(zip(("ll",) + TERM_GRADS, (ll,) + tuple(grads)), flag=flag)

    add("loglik_terms_grad" + tag, ["loglik_terms_grad"], lambda: _terms_inputs(12, Jr, Jc, fail), ref, run,
        {k: close() for k in ("ll",) + TERM_GRADS}, fail=fail, plan=("loglik_terms_grad", TERMS_MAPPING[Jr + 2 * Jc]))


_terms_row(0, 1, False)
_terms_row(1, 1, False)
_terms_row(0, 1, True)
_terms_row(0, 4, False)       # width 8: the fused one-lane kernels the benchmark's batch size takes
_terms_row(0, 4, True)


def _kernel_grad_build(name):
    """test_gpu_term_params.run_e2e's draw: one under-damped SHO term (width 2) or four of them (width 8)."""
    import term_params_ref as TP
    from test_gpu_term_params import make_case
    rng = np.random.default_rng(13)
    recs, P, _ = make_case(name, rng, D)
    widths = [TP.widths(r) for r in recs]
    x = np.sort(rng.uniform(0, N / 10.0, (D, N)), axis=1)
    return dict(_recs=recs, _Jr=sum(w[0] for w in widths), _Jc=sum(w[1] for w in widths), P=P, x=x, yerr=np.sqrt(rng.uniform(0.1, 0.3, (D, N))), y=np.sin(x) + 0.1 * rng.standard_normal((D, N)),
                jitter=rng.uniform(0.05, 0.4, D), mean=rng.uniform(-0.3, 0.3, D))


def _kernel_grad_ref(cpu, inp):
    from test_gpu_term_params import exact_series     # the complex step of the dense log-likelihood of the restatement
    want = [exact_series(inp["_recs"], inp["P"][b], inp["x"][b], inp["yerr"][b], inp["jitter"][b], inp["mean"][b], inp["y"][b]) for b in range(D)]
    return dict(ll=np.array([w[0] for w in want]), bP=np.stack([w[1] for w in want]), bjitter=np.array([w[2] for w in want]),
                bmean=np.array([w[3] for w in want]), flag=np.zeros(D, dtype=np.int64))


def _kernel_grad_run(ops, torch, T):
    prog = ops.TermProgram([dict(r, cols=tuple(r["cols"])) for r in T["_recs"]], T["P"].shape[1])
    out = tuple(nan_like(torch, *s) for s in ((B, T["P"].shape[1]), (B,), (B,), (B, N), (B, N), (B, N)))
    ll, (bP, bj, bm, bx, bdiag, by), flag = ops.loglik_kernel_grad(prog, T["P"], T["x"], T["yerr"], T["jitter"], T["mean"], T["y"], out=out)
    return dict(ll=ll, bP=bP, bjitter=bj, bmean=bm, flag=flag)


for _name, _width in (("sho/0/under", 2), ("sho4", 8)):
    add("loglik_kernel_grad[%s]" % _name, ["loglik_kernel_grad"], lambda name=_name: _kernel_grad_build(name), _kernel_grad_ref, _kernel_grad_run,
        {k: close() for k in ("ll", "bP", "bjitter", "bmean")}, symbols=(), plan=("kernel_grad", TERMS_MAPPING[_width]))


# -- term coefficients -----------------------------------------------------------------------------------------------------------
COEFS = ("ar", "cr", "ac", "bc", "cc", "dc")


def _term_coef_build(expr):
    import term_algebra_ref as A
    import term_params_ref as TP
    rng = np.random.default_rng(14)
    if expr:
        (recs, operations), P = A.draw_operation("product", "under", "real", rng, D)
        want = A.coefficients((recs, operations), P)[:6]
        cots = A.zero_inactive_rate_cotangents((recs, operations), P, [rng.standard_normal(w.shape) for w in want])
    else:
        (recs, P), operations = TP.draw("sho", rng, D, regime="under"), None
        want = TP.coefficients(recs, P)
        cots = TP.zero_inactive_rate_cotangents(recs, P, [rng.standard_normal(w.shape) for w in want])
    inp = dict(_recs=recs, _operations=operations, P=P, bshift=rng.standard_normal(D))
    inp.update({"b" + k: c for k, c in zip(COEFS, cots)})
    return inp


def _program(ops, T):
    recs = [dict(r, cols=tuple(r["cols"])) for r in T["_recs"]]
    if T["_operations"] is None:
        return ops.TermProgram(recs, T["P"].shape[1])
    return ops.TermExpr(recs, [dict(op=o["op"], a=o["a"], b=o["b"], col=o["col"]) for o in T["_operations"]], T["P"].shape[1])


def _term_coef_rows(expr):
    tag = "[expr]" if expr else "[program]"

    def ref(cpu, inp):
        import term_algebra_ref as A
        import term_params_ref as TP
        want = A.coefficients((inp["_recs"], inp["_operations"]), inp["P"]) if expr else TP.coefficients(inp["_recs"], inp["P"])
        out = dict(zip(COEFS, want[:6]), flag=np.zeros(D, dtype=np.int64))
        if expr:
            out["shift"] = np.asarray(want[6], dtype=float)
            assert not out["shift"].any()           # (no convolution: test_gpu_term_algebra.check_shift wants exact zeros)
        return out

    def run(ops, torch, T):
        prog = _program(ops, T)
        out = [nan_like(torch, B, w) for w in (prog.Jr, prog.Jr, prog.Jc, prog.Jc, prog.Jc, prog.Jc)]
        if expr:
            co, flag, shift = ops.term_coefficients(prog, T["P"], out=out, shift=nan_like(torch, B))
            return dict(zip(COEFS, co), flag=flag, shift=shift)
        co, flag = ops.term_coefficients(prog, T["P"], out=out)
        return dict(zip(COEFS, co), flag=flag)

    # test_gpu_term_params / test_gpu_term_algebra: 1e-13 of each series' largest entry per array
    crit = {k: rowmax(1e-13) for k in COEFS}
    crit["shift"] = EXACT
    add("term_coefficients" + tag, ["term_coefficients"] if not expr else [], lambda: _term_coef_build(expr), ref, run, crit,
        symbols=["c2_term_expr_coefficients" if expr else "c2_term_coefficients"])

    def ref_rev(cpu, inp):
        import term_algebra_ref as A
        import term_params_ref as TP
        cots = [inp["b" + k] for k in COEFS]
        if expr:
            return dict(bP=A.coefficients_rev((inp["_recs"], inp["_operations"]), inp["P"], cots, inp["bshift"]))
        return dict(bP=TP.coefficients_rev(inp["_recs"], inp["P"], cots))

    def run_rev(ops, torch, T):
        prog = _program(ops, T)
        kw = dict(bshift=T["bshift"]) if expr else {}
        return dict(bP=ops.term_coefficients_rev(prog, T["P"], [T["b" + k] for k in COEFS], out=nan_like(torch, B, T["P"].shape[1]), **kw))

    add("term_coefficients_rev" + tag, ["term_coefficients_rev"] if not expr else [], lambda: _term_coef_build(expr), ref_rev, run_rev,
        dict(bP=close()), symbols=["c2_term_expr_coefficients_rev" if expr else "c2_term_coefficients_rev"])


_term_coef_rows(False)
_term_coef_rows(True)


# -- jitter and mean ---------------------------------------------------------------------------------------------------------------
def _noise_build():
    rng = np.random.default_rng(15)
    ye, y, bd, by = (rng.standard_normal((D, N)) for _ in range(4))
    return dict(yerr=ye, y=y, bdiag=bd, by=by, jitter=rng.uniform(0.1, 1, D), mean=rng.standard_normal(D))


def _noise_apply_ref(cpu, inp):
    return dict(diag=inp["yerr"] ** 2 + inp["jitter"][:, None] ** 2, r=inp["y"] - inp["mean"][:, None])


def _noise_apply_run(ops, torch, T):
    return dict(zip(("diag", "r"), ops.noise_mean_apply(T["yerr"], T["jitter"], T["mean"], T["y"], out=(nan_like(torch, B, N), nan_like(torch, B, N)))))


# test_gpu_term_params.test_noise_mean_kernels: diag within 4 * 2^-53 relative, r the same bits as numpy
add("noise_mean_apply", ["noise_mean_apply"], _noise_build, _noise_apply_ref, _noise_apply_run, dict(diag=relative(4 * 2.0 ** -53), r=EXACT))


def _noise_rev_ref(cpu, inp):
    return dict(bjitter=2 * inp["jitter"] * inp["bdiag"].sum(1), bmean=-inp["by"].sum(1))


def _noise_rev_run(ops, torch, T):
    return dict(zip(("bjitter", "bmean"), ops.noise_mean_rev(T["jitter"], T["bdiag"], T["by"], out=(nan_like(torch, B), nan_like(torch, B)))))


# test_gpu_term_params.test_noise_mean_kernels: 1e-14 of 2 jitter sum |bdiag|, of sum |by|
add("noise_mean_rev", ["noise_mean_rev"], _noise_build, _noise_rev_ref, _noise_rev_run,
    dict(bjitter=lambda xo, keep, inp: 1e-14 * 2 * inp["jitter"] * np.abs(inp["bdiag"]).sum(1),
         bmean=lambda xo, keep, inp: 1e-14 * np.abs(inp["by"]).sum(1)))


# -- the 2-D extension ------------------------------------------------------------------------------------------------------------
KRON_GRADS = ("bt", "bc", "ba", "bU", "bV", "balpha", "bdiag", "by")
KRON_BANDS = 2


def _kron_build(fail, bands=KRON_BANDS):
    from oracle import dense
    t, c, a, U, V, alpha, diag, y, _ = dense.kron_synthetic(D, N, bands, 2)
    if fail:
        a[FAIL, N // 2] = -50.0       # a negative latent variance at one epoch (test_gpu_kron.test_kron_failures_and_invalid_diag)
    return dict(t=t, c=c, a=a, U=U, V=V, alpha=alpha, diag=diag, y=y)


def _kron_ref(cpu, inp):
    """test_gpu_kron.oracle_interleaved, keeping the oracle's flag instead of asserting it"""
    from oracle import dense
    lls, folded, flags = [], [], []
    for b in range(D):
        t2, c2, a2, U2, V2 = dense.kron_interleaved(inp["c"][b], inp["a"][b], inp["U"][b], inp["V"][b], inp["t"][b], inp["alpha"][b], inp["diag"][b])
        ll, g2, flag = cpu.loglik_grad(t2, c2, a2, U2, V2, np.ascontiguousarray(inp["y"][b].ravel()))
        lls.append(ll); flags.append(flag)
        folded.append(dense.kron_fold_gradients(g2, inp["a"][b], inp["U"][b], inp["V"][b], inp["alpha"][b]))
    out = dict(ll=np.array(lls), flag=np.array(flags))
    out.update({k: np.stack([f[i] for f in folded]) for i, k in enumerate(KRON_GRADS)})
    return out


def _totals(g, U, V):
    """test_gpu_kron.totals: (ba, bU, bV) -> the total derivatives along a = U.V"""
    return dict(bt=g["bt"], bc=g["bc"], tU=g["bU"] + g["ba"][..., None] * V, tV=g["bV"] + g["ba"][..., None] * U, balpha=g["balpha"],
                bdiag=g["bdiag"], by=g["by"])


def _kron_rows(method, fail, bands=KRON_BANDS):
    """bands = 2: lanes over the bands (k_kron_collapse[_rev]_b); 3, no power of two: the thread-per-epoch kernels"""
    tag = "[%s%s%s]" % (method, ",M=%d" % bands if bands != KRON_BANDS else "", ",fail" if fail else "")
    keys = ("t", "c", "a", "U", "V", "alpha", "diag", "y")
    collapsed = method == "collapsed"
    add("kron_loglik" + tag, ["kron_loglik"], lambda: _kron_build(fail, bands), lambda cpu, inp: {k: v for k, v in _kron_ref(cpu, inp).items() if k in ("ll", "flag")},
        lambda ops, torch, T: dict(zip(("ll", "flag"), ops.kron_loglik(*[T[k] for k in keys], method=method))), dict(ll=close()), fail=fail,
        bits=BITS_KRON if collapsed else None)

    def ref(cpu, inp):
        out = _kron_ref(cpu, inp)
        if collapsed:
            out = dict(_totals(out, inp["U"], inp["V"]), ll=out["ll"], flag=out["flag"])
        return out

    def run(ops, torch, T):
        ll, grads, flag = ops.kron_loglik_grad(*[T[k] for k in keys], method=method)
        g = dict(zip(KRON_GRADS, grads))
        if collapsed:
            g = _totals(g, T["U"], T["V"])
        return dict(g, ll=ll, flag=flag)

    if collapsed:     # another formulation than the oracle's: test_gpu_kron.COLLAPSED_FLOOR on the total derivatives
        crit = {k: close(1e-10, 5e-10) for k in ("bt", "bc", "tU", "tV", "balpha", "bdiag", "by")}
    else:
        crit = {k: close() for k in KRON_GRADS}
    crit["ll"] = close()
    # (bits: the totals are formed here from two outputs, so only ll of kron_loglik carries the bit rule)
    add("kron_loglik_grad" + tag, ["kron_loglik_grad"], lambda: _kron_build(fail, bands), ref, run, crit, fail=fail)


for _method in ("collapsed", "interleaved"):
    _kron_rows(_method, False)
    _kron_rows(_method, True)
_kron_rows("collapsed", False, 3)


# -- the trial sweeps and the projections ----------------------------------------------------------------------------------------
TRIALS, DRAWS, HARMONICS = 2, 2, 2


def _cases(make):
    return [make(100 + k) for k in range(D)]


def _whitened_row(name, width, make, trials_key, ref_fn, extra=(), count=()):
    """width: T's last axis at Q0 = 2 columns of Z0 (ops._TRIAL_TABLE; H (2 H + 1) + 2 H Q0 for the harmonics)"""
    keys = ("t", "c", "U", "W", "d", "Z0", trials_key) + tuple(extra)

    def build():
        return _stack(_cases(make), keys)

    def ref(cpu, inp):
        with np.errstate(all="ignore"):
            return dict(T=ref_fn(*[inp[k] for k in keys], *count))

    def run(ops, torch, T):
        return dict(T=getattr(ops, name)(*[T[k] for k in keys], *count, out=nan_like(torch, B, TRIALS, width)))

    add(name, [name], build, ref, run, dict(T=err()))


def _register_whitened():
    import harmonics_ref as HR
    import kepler_ref as KR
    import periodogram_ref as PR
    import shapes_ref as SR
    import transit_ref as TR
    _whitened_row("whitened_sinusoids", 7, lambda s: PR.case(s, N, 2, 1, F=TRIALS), "freq", PR.whitened_sinusoids_batched)
    _whitened_row("whitened_harmonics", HARMONICS * (2 * HARMONICS + 1) + 4 * HARMONICS, lambda s: HR.case(s, N, 2, 1, F=TRIALS), "freq", HR.whitened_harmonics_batched, count=(HARMONICS,))
    _whitened_row("whitened_transits", 3, lambda s: TR.case(s, N, 2, 1, K=TRIALS), "trials", TR.whitened_transits_batched)
    _whitened_row("whitened_keplerians", 7, lambda s: KR.case(s, N, 2, 1, K=TRIALS), "trials", KR.whitened_keplerians_batched)
    _whitened_row("whitened_shapes", 3, lambda s: SR.case(s, N, 2, 1, K=TRIALS), "trials", SR.whitened_shapes_batched, extra=("shapes",))


_register_whitened()


def _alpha(seed):
    return np.random.default_rng(seed).normal(size=(D, N, DRAWS))


def _projection_rows():
    import harmonic_significance_ref as HS
    import shapes_ref as SR
    import trial_projections_ref as TP

    for kind in TP.KINDS:
        key = TP.TRIALS_KEY[kind]

        def build(kind=kind, key=key):
            inp = _stack(_cases(lambda s: TP.case(kind, s, N, 2, 1, K=TRIALS)), ("t", key))
            inp["alpha"] = _alpha(16)
            return inp

        add("trial_projections[%s]" % kind, ["trial_projections"], build,
            lambda cpu, inp, kind=kind, key=key: dict(P=TP.projections_batched(kind, inp["t"], inp["alpha"], inp[key])),
            lambda ops, torch, T, kind=kind, key=key: dict(P=ops.trial_projections(kind, T["t"], T["alpha"], T[key],
                                                                                  out=nan_like(torch, B, TRIALS, TP.NCOL[kind], DRAWS))),
            dict(P=err()))

    def build_shape():
        inp = _stack(_cases(lambda s: SR.case(s, N, 2, 1, K=TRIALS)), ("t", "trials", "shapes"))
        inp["alpha"] = _alpha(17)
        return inp

    add("shape_projections", ["shape_projections"], build_shape,
        lambda cpu, inp: dict(P=SR.projections_batched(inp["t"], inp["alpha"], inp["trials"], inp["shapes"])),
        lambda ops, torch, T: dict(P=ops.shape_projections(T["t"], T["alpha"], T["trials"], T["shapes"], out=nan_like(torch, B, TRIALS, 1, DRAWS))),
        dict(P=err()))

    H, NC, P0 = HARMONICS, 2 * HARMONICS, 1

    def build_harm():
        inp = _stack(_cases(lambda s: HS.case(s, N, 2, P0, TRIALS, H)), ("t", "freq"))
        inp["alpha"] = _alpha(18)
        # a well-conditioned packed lower factor, the null columns' products and the null fit's coefficients: inputs only
        rng = np.random.default_rng(19)
        Lm = 0.1 * rng.normal(size=(D, TRIALS, H * (2 * H + 1)))
        for i in range(NC):
            Lm[..., i * (i + 1) // 2 + i] = rng.uniform(1.0, 2.0, (D, TRIALS))
        inp.update(Lm=Lm, Xt=0.3 * rng.normal(size=(D, TRIALS, NC, P0)), V=rng.normal(size=(D, P0, DRAWS)))
        return inp

    add("harmonic_projections", ["harmonic_projections"], build_harm,
        lambda cpu, inp: dict(P=HS.projections_batched(inp["t"], inp["alpha"], inp["freq"], H)),
        lambda ops, torch, T: dict(P=ops.harmonic_projections(T["t"], T["alpha"], T["freq"], H, out=nan_like(torch, B, TRIALS, NC, DRAWS))),
        dict(P=err()))

    def ref_chi2(cpu, inp):   # the restated lines on the restated projections
        P = HS.projections_batched(inp["t"], inp["alpha"], inp["freq"], H)
        return dict(D=np.stack([HS.null_chi2(P[b], inp["Lm"][b], inp["Xt"][b], inp["V"][b]) for b in range(D)]))

    add("harmonic_null_chi2", ["harmonic_null_chi2"], build_harm, ref_chi2,
        lambda ops, torch, T: dict(D=ops.harmonic_null_chi2(T["t"], T["alpha"], T["freq"], H, T["Lm"], T["Xt"], T["V"],
                                                            out=nan_like(torch, B, TRIALS, DRAWS))),
        dict(D=err()))


_projection_rows()


# -- streaming updates ---------------------------------------------------------------------------------------------------------
HEAD_ROWS = 4                                        # rows absorbed before the M new ones
COUNTS = np.array([0, 1, 2, 2, 1, 0, 2], dtype=np.int32)     # ragged: rows m >= count are neither read nor written


def _filter_build(J, fail=False):
    import filter_ref as F
    ds = _draws(20 + J, HEAD_ROWS + M, J)
    inp = {k: np.stack([d[k][HEAD_ROWS:] for d in ds]) for k in "taUVy"}
    inp["c"] = np.stack([d["c"] for d in ds])
    st0, dd, WW, zz = [], [], [], []
    for d in ds:
        st = F.empty(J)
        st, _, _, _, flag = F.append(st, d["c"], *(d[k][:HEAD_ROWS] for k in "taUVy"))
        assert flag == 0
        st0.append(st)
        dw, Ww = F.factor(d["t"], d["c"], d["a"], d["U"], d["V"])
        dd.append(dw[HEAD_ROWS:]); WW.append(Ww[HEAD_ROWS:]); zz.append(F.solve_lower(d["t"], d["c"], d["U"], Ww, d["y"])[HEAD_ROWS:])
    inp.update(state=np.stack(st0), count=COUNTS.copy(), d=np.stack(dd), W=np.stack(WW), z=np.stack(zz))
    if fail:
        inp["a"][FAIL, 0] = -1.0                    # (series FAIL takes two rows: its first one fails)
    return inp


def _rows_to(x, k, shape):
    out = np.full(shape, np.nan)
    out[:k] = x[:k]
    return out


def _state_parts(st, J):
    return dict(head=st[:, :2], sums=st[:, 2:4], F=st[:, 4:4 + J], S=st[:, 4 + J:])


def _filter_rows(J):
    import filter_ref as F
    import filter_rev_ref as FR

    def ref_append(cpu, inp):
        st, d, W, z, flag = [], [], [], [], []
        for b in range(D):
            k = int(inp["count"][b])
            s, dk, Wk, zk, f = F.append(inp["state"][b], inp["c"][b], *(inp[x][b][:k] for x in "taUVy"))
            st.append(s); flag.append(f)
            d.append(_rows_to(dk, k, (M,))); W.append(_rows_to(Wk, k, (M, J))); z.append(_rows_to(zk, k, (M,)))
        return dict(_state_parts(np.stack(st), J), d=np.stack(d), W=np.stack(W), z=np.stack(z), flag=np.array(flag))

    def run_append(ops, torch, T):
        SW = T["state"].shape[1]
        st, d, W, z, flag = ops.filter_append(T["state"], T["t"], T["c"], T["a"], T["U"], T["V"], T["y"], count=T["count"],
                                              out=nan_like(torch, B, SW), d=nan_like(torch, B, M), W=nan_like(torch, B, M, J),
                                              z=nan_like(torch, B, M))
        return dict(_state_parts(st, J), d=d, W=W, z=z, flag=flag)

    # test_gpu_filter.check_state: t_last and n exact, the sums, F and S each by the standing criterion
    state_crit = dict(head=EXACT, sums=err(), F=err(), S=err())
    for fail in (False, True):
        add("filter_append[J=%d%s]" % (J, ",fail" if fail else ""), ["filter_append"], lambda fail=fail: _filter_build(J, fail), ref_append,
            run_append, dict(state_crit, d=err(), W=err(), z=err()), fail=fail, ragged=True)

    def ref_absorb(cpu, inp):
        st = [F.absorb(inp["state"][b], inp["c"][b], *(inp[x][b][:int(inp["count"][b])] for x in "tWdz")) for b in range(D)]
        return _state_parts(np.stack(st), J)

    add("filter_absorb[J=%d]" % J, ["filter_absorb"], lambda: _filter_build(J), ref_absorb,
        lambda ops, torch, T: _state_parts(ops.filter_absorb(T["state"], T["t"], T["c"], T["W"], T["d"], T["z"], count=T["count"],
                                                             out=nan_like(torch, B, T["state"].shape[1])), J), state_crit, ragged=True)

    def build_forecast():
        inp = _filter_build(J)
        inp["count"] = (COUNTS + 1).astype(np.int32)      # 1 .. 3 = M query rows, all from the same state
        inp["_ymax"] = _amax(np.stack([d["y"] for d in _draws(20 + J, HEAD_ROWS + M, J)]))
        return inp

    def ref_forecast(cpu, inp):
        mu, var = [], []
        for b in range(D):
            k = int(inp["count"][b])
            m, v = F.forecast(inp["state"][b], inp["c"][b], inp["t"][b][:k], inp["a"][b][:k], inp["U"][b][:k])
            mu.append(_rows_to(m, k, (M,))); var.append(_rows_to(v, k, (M,)))
        return dict(mu=np.stack(mu), var=np.stack(var))

    def mu_crit(xo, keep, inp):   # test_gpu_filter.test_forecast_against_dense_conditioning: the floor max(|mu_o|, |y|)
        return err(floor=max(_amax(xo), inp["_ymax"]))(xo, keep)

    add("filter_forecast[J=%d]" % J, ["filter_forecast"], build_forecast, ref_forecast,
        lambda ops, torch, T: dict(zip(("mu", "var"), ops.filter_forecast(T["state"], T["t"], T["c"], T["a"], T["U"], count=T["count"],
                                                                          mu=nan_like(torch, B, M), var=nan_like(torch, B, M)))),
        dict(mu=mu_crit, var=err()), ragged=True)

    rev_names = ("bstate_in", "bt", "bc", "ba", "bU", "bV", "by")

    def build_rev():
        inp = _filter_build(J)
        # the forward call's own rows, by the restatement: what the reverse reads
        d, W, z = np.zeros((D, M)), np.zeros((D, M, J)), np.zeros((D, M))
        for b in range(D):
            k = int(inp["count"][b])
            _, dk, Wk, zk, f = F.append(inp["state"][b], inp["c"][b], *(inp[x][b][:k] for x in "taUVy"))
            assert f == 0
            d[b, :k], W[b, :k], z[b, :k] = dk, Wk, zk
        rng = np.random.default_rng(21 + J)
        inp.update(d=d, W=W, z=z, fflag=np.zeros(D, dtype=np.int32), bstate=rng.normal(size=(D, F.state_words(J))),
                   bd=rng.normal(size=(D, M)), bW=rng.normal(size=(D, M, J)), bz=rng.normal(size=(D, M)))
        return inp

    def ref_rev(cpu, inp):
        out = [FR.append_rev(inp["state"][b], inp["c"][b], inp["t"][b], inp["U"][b], inp["W"][b], inp["d"][b], inp["z"][b], 0,
                             inp["bstate"][b], inp["bd"][b], inp["bW"][b], inp["bz"][b], count=int(inp["count"][b])) for b in range(D)]
        res = {k: np.stack([o[i] for o in out]) for i, k in enumerate(rev_names) if i}
        bs = np.stack([o[0] for o in out])
        res.update(bhead=bs[:, :4], bF=bs[:, 4:4 + J], bS=bs[:, 4 + J:], ws=np.stack([o[7] for o in out]))
        return res

    def run_rev(ops, torch, T):
        SW = T["state"].shape[1]
        out = tuple(nan_like(torch, *s) for s in ((B, SW), (B, M), (B, J), (B, M), (B, M, J), (B, M, J), (B, M)))
        ws = nan_like(torch, B, M, J + J * J)
        got = ops.filter_append_rev(T["state"], T["t"], T["c"], T["U"], T["W"], T["d"], T["z"], T["fflag"], T["bstate"], T["bd"], T["bW"],
                                    T["bz"], count=T["count"], ws=ws, out=out)
        res = dict(zip(rev_names[1:], got[1:]))
        res.update(bhead=got[0][:, :4], bF=got[0][:, 4:4 + J], bS=got[0][:, 4 + J:], ws=ws)
        return res

    # test_gpu_filter_rev.check / check_outputs: an all-zero expectation takes the scale of the unit-normal cotangents
    crit = {k: err(zero_floor=1.0) for k in rev_names[1:] + ("bhead", "bF", "bS", "ws")}
    # (ws: the rows the forward call took -- what lies beyond count is scratch)
    add("filter_append_rev[J=%d]" % J, ["filter_append_rev"], build_rev, ref_rev, run_rev, crit, where_ref=("ws",), ragged=True)


for _J in WIDTHS:
    _filter_rows(_J)


def _filter_init_run(ops, torch, T):
    return dict(state=ops.filter_init(B, 2, "cuda"))


add("filter_init", ["filter_init"], lambda: dict(), lambda cpu, inp: dict(state=np.zeros((D, 4 + 2 + 4))), _filter_init_run,
    dict(state=EXACT), symbols=())


# ---- where the other public names stand ----------------------------------------------------------------------------------------
# name -> "file::test": an existing test that runs the entry point beyond 65535 series
COVERED_ELSEWHERE = {
    "whitened_gram": "test_gpu_linear_model.py::test_batch_beyond_65535",
    "c2_whitened_gram": "test_gpu_linear_model.py::test_batch_beyond_65535",
    "inverse_diag": "test_gpu_inverse_diag.py::test_seventy_thousand_series",
    "c2_inverse_diag": "test_gpu_inverse_diag.py::test_seventy_thousand_series",
    "c2_inverse_diag_fwd": "test_gpu_inverse_diag_rev.py::test_seventy_thousand_series",
    "inverse_diag_rev": "test_gpu_inverse_diag_rev.py::test_seventy_thousand_series",
    "c2_inverse_diag_rev": "test_gpu_inverse_diag_rev.py::test_seventy_thousand_series",
    "explained_variance": "test_gpu_predict_at.py::test_seventy_thousand_series",
    "c2_explained_variance": "test_gpu_predict_at.py::test_seventy_thousand_series",
    "c2_explained_variance_fwd": "test_gpu_explained_variance_rev.py::test_seventy_thousand_series",
    "explained_variance_rev": "test_gpu_explained_variance_rev.py::test_seventy_thousand_series",
    "c2_explained_variance_rev": "test_gpu_explained_variance_rev.py::test_seventy_thousand_series",
    "prior_draw": "test_gpu_sample_at.py::test_seventy_thousand_series",
    "c2_prior_draw": "test_gpu_sample_at.py::test_seventy_thousand_series",
    "general_matmul_lower_rev": "test_gpu_general_rev.py::test_seventy_thousand_series",
    "c2_general_matmul_lower_rev": "test_gpu_general_rev.py::test_seventy_thousand_series",
    "general_matmul_upper_rev": "test_gpu_general_rev.py::test_seventy_thousand_series",
    "c2_general_matmul_upper_rev": "test_gpu_general_rev.py::test_seventy_thousand_series",
    "noise_mean_shift_apply": "test_gpu_term_algebra.py::test_noise_mean_shift_kernels",
    "c2_noise_mean_shift_apply": "test_gpu_term_algebra.py::test_noise_mean_shift_kernels",
    "noise_mean_shift_rev": "test_gpu_term_algebra.py::test_noise_mean_shift_kernels",
    "c2_noise_mean_shift_rev": "test_gpu_term_algebra.py::test_noise_mean_shift_kernels",
    "filter_forecast_rev": "test_gpu_filter_stream_rev.py::test_large_batch",
    "c2_filter_forecast_rev": "test_gpu_filter_stream_rev.py::test_large_batch",
    "filter_absorb_rev": "test_gpu_filter_stream_rev.py::test_large_batch",
    "c2_filter_absorb_rev": "test_gpu_filter_stream_rev.py::test_large_batch",
    "filter_draw": "test_gpu_filter_draw.py::test_large_batch",
    "c2_filter_draw": "test_gpu_filter_draw.py::test_large_batch",
}

# name -> why it has no batch axis to take beyond 65535
NO_BATCH_AXIS = {
    "loglik_grad_workspace": "a workspace-size query", "loglik_kernel_workspace": "allocates the buffers of loglik_kernel_grad",
    "TermProgram": "a description of the kernel, no series", "TermExpr": "a description of the kernel, no series",
    "c2_version": "a string", "c2_device_count": "a count of devices", "c2_last_error": "a string",
    "c2_loglik_grad_workspace_bytes": "a workspace-size query", "c2_kron_loglik_workspace_bytes": "a workspace-size query",
    "c2_loglik_terms_workspace_bytes": "a workspace-size query", "c2_term_expr_workspace_bytes": "a workspace-size query",
    "c2_get_celerite_matrices_rev_workspace_bytes": "a workspace-size query",
    "c2_filter_state_words": "a size query", "c2_filter_rev_workspace_words": "a size query",
    "filter_state_words": "a size query", "filter_rev_workspace_words": "a size query",
    "filter_draw_chunk": "a size query", "c2_filter_draw_chunk": "a size query",
    "c2_set_option": "the option table", "c2_get_option": "the option table", "c2_option_count": "the option table",
    "c2_option_info": "the option table", "c2_options_reload_env": "the option table",
    "c2h_release_thread_cache": "the host layer's staging cache",
}
# the host drop-in takes ONE series per call (N, J, nrhs: no B)
NO_BATCH_AXIS.update({"c2h_" + n: "the host drop-in: one series per call" for n in (
    "factor", "solve_lower", "solve_upper", "matmul_lower", "matmul_upper", "general_matmul_lower", "general_matmul_upper", "factor_rev",
    "solve_lower_rev", "solve_upper_rev", "matmul_lower_rev", "matmul_upper_rev", "get_celerite_matrices")})


def table_names():
    names = set()
    for row in ROWS:
        names.update(row.ops)
        names.update(row.symbols)
    return names


# ---- the launchers' own plans (host functions: no device needed) -----------------------------------------------------------
def plan_hooks():
    import ctypes
    from celerite2_amd import _lib

    lib = ctypes.CDLL(_lib.LIB_PATH)
    i64, out = ctypes.c_int64, [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_size_t)]
    lib.c2_internal_loglik_grad_plan.restype, lib.c2_internal_loglik_grad_plan.argtypes = ctypes.c_int, [i64] * 3 + [ctypes.c_int] * 2 + out
    lib.c2_internal_loglik_terms_plan.restype, lib.c2_internal_loglik_terms_plan.argtypes = ctypes.c_int, [i64] * 4 + [ctypes.c_int] + out
    lib.c2_internal_general_chunks_plan.restype, lib.c2_internal_general_chunks_plan.argtypes = i64, [i64] * 3
    return lib


def mapping_of(raw, row, inp):
    """The mapping (c2::Lanes; tests/test_workspace_plan.py names them) the launcher's plan reports for the row's call at B
    series -- for the general products the chunk length, 0 = no chunks along time."""
    import ctypes
    m, need = ctypes.c_int(), ctypes.c_size_t()
    hook = row.plan[0]
    if hook == "loglik_grad":
        n, J = inp["U"].shape[1:]
        seen = set()
        for aligned16 in (0, 1):
            assert raw.c2_internal_loglik_grad_plan(B, n, J, 1, aligned16, ctypes.byref(m), ctypes.byref(need)) == 0
            seen.add(m.value)
        assert len(seen) == 1, (row.id, seen)
        return m.value
    if hook == "general_chunks":
        return int(raw.c2_internal_general_chunks_plan(B, inp["V"].shape[1], inp["Y"].shape[2]))
    if hook == "kernel_grad":
        n, Jr, Jc, grad = inp["x"].shape[1], inp["_Jr"], inp["_Jc"], 1
    else:
        n, Jr, Jc, grad = inp["x"].shape[1], inp["ar"].shape[1], inp["ac"].shape[1], int(hook.endswith("grad"))
    assert raw.c2_internal_loglik_terms_plan(B, n, Jr, Jc, grad, ctypes.byref(m), ctypes.byref(need)) == 0
    return m.value
