# -*- coding: utf-8 -*-
"""GPU checks of the ragged batches (celerite2_amd/packed.py over csrc/c2_packed.hip): values, factors and all six gradients
of series of different lengths in one packed call.

Reference: the CPU oracle called ONCE PER SERIES on that series' own length (oracle.loglik_grad_batched with B = 1;
factor_flag + solve_lower for d, W, z).  Inputs: parity_cases.problem.  Criterion: parity_cases.close -- 1e-10 relative per
element plus 1e-12 of the array's largest entry -- per series and per array, no series left out.  Everything that must not
depend on something (the order, the neighbours, what the buffers held) is compared to the bit."""
import math

import numpy as np
import pytest

from parity_cases import close, dev, problem

pytestmark = pytest.mark.gpu
WIDTHS = (1, 2, 3, 5, 8, 16, 17, 32)
BATCHES = (1, 3, 65, 130)
NMAX = 150
GRADS = ("bt", "bc", "ba", "bU", "bV", "by")


@pytest.fixture(scope="module")
def packed():
    import torch
    from celerite2_amd import packed as p
    assert torch.cuda.is_available()
    return p


def mixed_lengths(B, C):
    """150 at every position a group of lanes can have in a wavefront (the even slots of the first 64 series, the odd ones of
    the next 64), the smallest lengths that can go wrong between them: 0, 1, 2 and C-1, C, C+1, 2C+1 around the checkpoints."""
    small = (0, 1, 2, C - 1, C, C + 1, 2 * C + 1)
    out = []
    for b in range(B):
        full = (b % 2 == 0) if (b // 64) % 2 == 0 else (b % 2 == 1)
        out.append(NMAX if full else small[(b // 2) % len(small)])
    return out


def pack_rect(packed, arrays, lengths, take=None):
    """Rows [:lengths[b]] of series take[b] (default b) of rectangular (B, N, ...) host arrays, packed; -> (pk, device arrays)."""
    import torch
    take = range(len(lengths)) if take is None else take
    cat = [np.concatenate([x[s, :n] for s, n in zip(take, lengths)], axis=0) for x in arrays]
    t, *rest = dev(*cat)
    return packed.Packed(t, lengths), rest


_REF = {}


def reference(oracle, J, shared=False):
    """problem(None, 130, 150, J) and the oracle's answers series by series at mixed_lengths (computed once per width and
    kept unchanged).  shared: every series is a prefix of series 0, so that one c (J,) serves the batch."""
    key = (J, shared)
    if key not in _REF:
        C = math.isqrt(NMAX - 1) + 1
        lengths = mixed_lengths(130, C)
        t, c, a, U, V, y = problem(None, 130, NMAX, J)
        take = [0] * 130 if shared else list(range(130))
        memo, want = {}, []
        for b, n in enumerate(lengths):
            s = take[b]
            if (s, n) not in memo:
                memo[(s, n)] = series_reference(oracle, t[s, :n], c[s], a[s, :n], U[s, :n], V[s, :n], y[s, :n])
            want.append(memo[(s, n)])
        _REF[key] = dict(C=C, lengths=lengths, take=take, arrays=(t, a, U, V, y), c=c[0] if shared else c, want=want)
    return _REF[key]


def series_reference(oracle, t, c, a, U, V, y):
    n, J = U.shape
    if n == 0:
        z1, z2 = np.zeros(0), np.zeros((0, J))
        return dict(ll=0.0, flag=0, d=z1, W=z2, z=z1, bt=z1, bc=np.zeros(J), ba=z1, bU=z2, bV=z2, by=z1)
    cc = lambda x: np.ascontiguousarray(x)
    t, c, a, U, V, y = map(cc, (t, c, a, U, V, y))
    ll, grads, flag = oracle.loglik_grad_batched(t[None], c[None], a[None], U[None], V[None], y[None])
    d, W = np.empty(n), np.empty((n, J))
    assert oracle.factor_flag(t, c, a, U, V, d, W, np.empty((n, J, J))) == 0 and int(flag[0]) == 0
    z = np.empty((n, 1))
    oracle.solve_lower(t, c, U, W, cc(y[:, None]), z)
    out = dict(ll=float(ll[0]), flag=0, d=d, W=W, z=z[:, 0])
    out.update({k: g[0] for k, g in zip(GRADS, grads)})
    return out


def check_series(key, pk, want, ll, flag, grads=None, dWz=None):
    """Every series of a call against its reference, array by array."""
    assert flag.cpu().tolist() == [w["flag"] for w in want], key
    close(ll, np.array([w["ll"] for w in want]))
    got = {}
    if grads is not None:
        got.update(zip(GRADS, grads))
    if dWz is not None:
        got.update(zip("dWz", dWz))
    off = pk.offsets.tolist()
    for k, arr in got.items():
        arr = arr.cpu().numpy()   # (one copy per array)
        for b, w in enumerate(want):
            x = arr[b] if k == "bc" else arr[off[b]:off[b + 1]]
            assert x.shape == w[k].shape, (key, k, b)
            if x.size:
                try:
                    close(x, w[k])
                except AssertionError as e:
                    raise AssertionError("%s: %s of series %d (length %d): %s" % (key, k, b, pk.lengths[b], e))


# ---- values and gradients --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J", WIDTHS)
def test_values_and_gradients(oracle, packed, J):
    """Every group size, partial wavefronts, lengths on both sides of every checkpoint, 0, 1, 2 and 150 in every position of a
    wavefront; c per series and shared: ll, flag, d, W, z and the six gradients of every series."""
    for shared in (False, True):
        ref = reference(oracle, J, shared)
        assert packed.checkpoint_interval(NMAX) == ref["C"] == 13
        for B in BATCHES:
            key = (J, B, shared)
            lengths = ref["lengths"][:B]
            assert lengths[0] == NMAX
            pk, (a, U, V, y) = pack_rect(packed, ref["arrays"], lengths, ref["take"][:B])
            c, = dev(ref["c"] if shared else ref["c"][:B])
            want = ref["want"][:B]
            for order in (None, "sorted"):   # None: the positions as mixed_lengths lays them out
                ll, flag, d, W, z = packed.loglik(pk, c, a, U, V, y, factor=True, order=order)
                check_series(key, pk, want, ll, flag, dWz=(d, W, z))
                ll0, flag0 = packed.loglik(pk, c, a, U, V, y, order=order)
                assert np.array_equal(ll0.cpu().numpy(), ll.cpu().numpy()) and flag0.tolist() == flag.tolist()
                ll, grads, flag = packed.loglik_grad(pk, c, a, U, V, y, order=order)
                assert tuple(grads[1].shape) == (B, J)
                check_series(key, pk, want, ll, flag, grads=grads)
                assert np.array_equal(ll0.cpu().numpy(), ll.cpu().numpy())   # the two forward passes are one recursion


def test_equal_lengths_against_the_rectangle(oracle, packed):
    """B = 5 series of 150 rows: the packed call against ops.loglik_grad on the rectangle, and both against the oracle."""
    from celerite2_amd import ops
    for J in (2, 8, 17):
        B = 5
        t, c, a, U, V, y = problem(None, B, NMAX, J)
        ll_r, grads_r, flag_r = ops.loglik_grad(*dev(t, c, a, U, V, y))
        pk, (ap, Up, Vp, yp) = pack_rect(packed, (t, a, U, V, y), [NMAX] * B)
        ll, grads, flag = packed.loglik_grad(pk, dev(c)[0], ap, Up, Vp, yp)
        assert flag.tolist() == flag_r.tolist() == [0] * B
        close(ll, ll_r.cpu().numpy())
        for k, g, gr in zip(GRADS, grads, grads_r):
            g = g if k == "bc" else pk.to_padded(g)
            for b in range(B):
                close(g[b], gr[b].cpu().numpy())
        want = [series_reference(oracle, t[b], c[b], a[b], U[b], V[b], y[b]) for b in range(B)]
        check_series((J, "rect"), pk, want, ll, flag, grads=grads)


# ---- what the results must not depend on -------------------------------------------------------------------------------------
def _all_outputs(packed, pk, c, a, U, V, y, order):
    ll, flag, d, W, z = packed.loglik(pk, c, a, U, V, y, factor=True, order=order)
    ll2, grads, flag2 = packed.loglik_grad(pk, c, a, U, V, y, order=order)
    return [ll, flag, d, W, z, ll2, flag2, *grads]


@pytest.mark.parametrize("J", (3, 8))
def test_order_changes_no_bit(oracle, packed, J):
    import torch
    ref = reference(oracle, J)
    pk, (a, U, V, y) = pack_rect(packed, ref["arrays"], ref["lengths"])
    c, = dev(ref["c"])
    perm = torch.from_numpy(np.random.default_rng(J).permutation(130).astype(np.int32)).cuda()
    base = _all_outputs(packed, pk, c, a, U, V, y, None)
    assert all(bool(torch.isfinite(x).all()) for x in base if x.dtype == torch.float64)
    for order in (None, "sorted", "auto", perm, pk.order):
        again = _all_outputs(packed, pk, c, a, U, V, y, order)
        for i, (x, x0) in enumerate(zip(again, base)):
            assert torch.equal(x, x0), (J, i)


@pytest.mark.parametrize("J", (2, 8))
def test_neighbours_change_no_bit(oracle, packed, J):
    """65 series, then the same with series 7 and 40 cut to 0 and 1 rows and the arrays re-packed: every other series' outputs
    are equal to the bit."""
    import torch
    ref = reference(oracle, J)
    l0 = list(ref["lengths"][:65])
    l1 = list(l0); l1[7], l1[40] = 0, 1
    assert l0[7] != 0 and l0[40] == NMAX
    c, = dev(ref["c"][:65])
    runs = []
    for lengths in (l0, l1):
        pk, (a, U, V, y) = pack_rect(packed, ref["arrays"], lengths)
        out = _all_outputs(packed, pk, c, a, U, V, y, None)
        runs.append([x if x.shape[0] == 65 else pk.unpack(x) for x in out])
    for i, (x0, x1) in enumerate(zip(*runs)):
        for b in range(65):
            if b not in (7, 40):
                assert torch.equal(x0[b], x1[b]), (J, i, b)


def _raw(packed, pk, c, a, U, V, y, fill):
    """Both entry points on buffers of the caller's, every one of them filled with `fill` first."""
    import torch
    from celerite2_amd import ops
    fns = packed._load()
    B, R, J = pk.B, pk.R, U.shape[1]
    f64 = lambda *s: torch.full(s, fill, dtype=torch.float64, device="cuda")
    i32 = lambda: torch.full((B,), -77, dtype=torch.int32, device="cuda")
    ll, flag, d, W, z = f64(B), i32(), f64(R), f64(R, J), f64(R)
    assert fns["c2_packed_loglik"](B, R, J, pk.offsets, pk.order, pk.t, c, J, a, U, V, y, ll, flag, d, W, z, ops._stream()) == 0
    ll2, flag2 = f64(B), i32()
    grads = [f64(R), f64(B, J), f64(R), f64(R, J), f64(R, J), f64(R)]
    work = packed.workspace(pk, J).fill_(fill)
    assert fns["c2_packed_loglik_grad"](B, R, pk.n_max, J, pk.offsets, pk.order, pk.t, c, J, a, U, V, y, ll2, *grads, flag2, work,
                                        work.numel() * 8, ops._stream()) == 0
    torch.cuda.synchronize()
    return [ll, flag, d, W, z, ll2, flag2, *grads]


@pytest.mark.parametrize("J", (5, 16))
def test_dirty_memory(oracle, packed, J):
    """Outputs and work pre-filled with 7.0 and with NaN: equal bits, and every element of every output written (no NaN, no
    sentinel flag left; the inputs have no 7.0 to hide behind -- the two runs agree)."""
    import torch
    ref = reference(oracle, J)
    pk, (a, U, V, y) = pack_rect(packed, ref["arrays"], ref["lengths"])
    c, = dev(ref["c"])
    r7, rn = _raw(packed, pk, c, a, U, V, y, 7.0), _raw(packed, pk, c, a, U, V, y, float("nan"))
    for i, (x, x0) in enumerate(zip(rn, r7)):
        assert torch.equal(x, x0), (J, i)
        assert bool(torch.isfinite(x).all()) if x.dtype == torch.float64 else bool((x == 0).all()), (J, i)
    check_series((J, "dirty"), pk, ref["want"], rn[5], rn[6], grads=rn[7:], dWz=rn[2:5])


# ---- failure ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J", (1, 8))
def test_failure_is_contained(oracle, packed, J):
    """A negative diagonal at row 3 of one series in the middle of a wavefront: its flag, ll = -inf and NaN where the header
    says; its 63 neighbours keep their bits.  A NaN pivot passes."""
    import torch
    B, bad = 64, 35
    t, c, a, U, V, y = problem(None, B, 40, J)
    lengths = [40 - (b % 5) for b in range(B)]
    cd, = dev(c)
    pk, (ad, Ud, Vd, yd) = pack_rect(packed, (t, a, U, V, y), lengths)
    good = _all_outputs(packed, pk, cd, ad, Ud, Vd, yd, None)
    assert good[1].tolist() == [0] * B
    row = int(pk.offsets[bad]) + 2
    for value in (-5.0, float("nan")):
        a2 = ad.clone(); a2[row] = value
        out = _all_outputs(packed, pk, cd, a2, Ud, Vd, yd, None)
        ll, flag, d, W, z, ll2, flag2, *grads = out
        for i, (x, x0) in enumerate(zip(out, good)):   # the neighbours, to the bit
            xs, x0s = (x, x0) if x.shape[0] == B else (pk.unpack(x), pk.unpack(x0))
            for b in range(B):
                if b != bad:
                    assert torch.equal(xs[b], x0s[b]), (J, value, i, b)
        if value != value:   # a NaN pivot passes: no flag, NaN from that row on
            assert flag[bad] == 0 and flag2[bad] == 0 and bool(torch.isnan(ll[bad])) and bool(torch.isnan(ll2[bad]))
            continue
        assert flag[bad] == 3 and flag2[bad] == 3
        assert ll[bad] == -float("inf") and ll2[bad] == -float("inf")
        db, Wb, zb = (pk.unpack(x)[bad] for x in (d, W, z))
        d0, W0, z0 = (pk.unpack(x)[bad] for x in good[2:5])
        assert torch.equal(db[:2], d0[:2]) and torch.equal(Wb[:2], W0[:2]) and torch.equal(zb[:2], z0[:2])
        assert db[2] <= 0.0
        assert bool(torch.isnan(db[3:]).all()) and bool(torch.isnan(Wb[2:]).all()) and bool(torch.isnan(zb[2:]).all())
        for k, g in zip(GRADS, grads):
            gb = g[bad] if k == "bc" else pk.unpack(g)[bad]
            assert gb.numel() and bool(torch.isnan(gb).all()), (J, k)


# ---- series boundaries ----------------------------------------------------------------------------------------------------------
def test_no_decay_across_a_series_boundary(packed):
    """Each series starts 1e6 below the last time of the one before it, rates up to 10: exp of that difference would be inf.
    Everything stays finite and every series has the bits it has when packed alone."""
    import torch
    lengths = [3, 40, 0, 17, 150, 1]
    B, J = len(lengths), 2
    t, _, _, _, _, y = problem(None, B, NMAX, 2)
    t = t - 1.0e6 * (np.arange(B)[:, None] + 1) - t.max()
    rng = np.random.default_rng(3)
    ar = rng.uniform(0.3, 1.0, (B, J))
    c = np.stack([rng.uniform(0.2, 1.0, B), np.full(B, 10.0)], axis=1)
    U = np.repeat(ar[:, None, :], NMAX, axis=1); V = np.ones((B, NMAX, J))
    a = ar.sum(1)[:, None] + rng.uniform(0.1, 0.3, (B, NMAX))
    pk, (ad, Ud, Vd, yd) = pack_rect(packed, (t, a, U, V, y), lengths)
    assert float(pk.t[2] - pk.t[3]) > 9.0e5   # the boundary between series 0 and 1
    cd, = dev(c)
    out = _all_outputs(packed, pk, cd, ad, Ud, Vd, yd, "sorted")
    assert all(bool(torch.isfinite(x).all()) for x in out if x.dtype == torch.float64) and out[1].tolist() == [0] * B
    for b, n in enumerate(lengths):
        p1, (a1, U1, V1, y1) = pack_rect(packed, (t, a, U, V, y), [n], take=[b])
        alone = _all_outputs(packed, p1, cd[b:b + 1].contiguous(), a1, U1, V1, y1, None)
        for i, (x, x1) in enumerate(zip(out, alone)):
            xb = x[b:b + 1] if x.shape[0] == B else pk.unpack(x)[b]
            assert torch.equal(xb, x1), (b, i)


# ---- beyond 65535 series ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J", (2, 8))
def test_batch_beyond_65535(oracle, packed, J):
    """B = 70000: seven distinct series with lengths 0 .. 5 (and 0 again), replicated; every series against the oracle's seven
    answers."""
    import torch
    B, rep = 70000, 10000
    l7 = [0, 1, 2, 3, 4, 5, 0]
    t, c, a, U, V, y = problem(None, 7, 5, J)
    want = [series_reference(oracle, t[s, :n], c[s], a[s, :n], U[s, :n], V[s, :n], y[s, :n]) for s, n in enumerate(l7)]
    cat = [np.concatenate([x[s, :n] for s, n in enumerate(l7)], axis=0) for x in (t, a, U, V, y)]
    td, ad, Ud, Vd, yd = dev(*[np.tile(x, (rep,) + (1,) * (x.ndim - 1)) for x in cat])
    cd, = dev(np.tile(c, (rep, 1)))
    pk = packed.Packed(td, l7 * rep)
    assert pk.B == B and pk.R == 15 * rep and packed.checkpoint_interval(pk.n_max) == 3
    ll, flag, d, W, z = packed.loglik(pk, cd, ad, Ud, Vd, yd, factor=True)
    ll2, grads, flag2 = packed.loglik_grad(pk, cd, ad, Ud, Vd, yd)
    assert not bool(flag.any()) and not bool(flag2.any()) and torch.equal(ll, ll2)
    close(ll.reshape(rep, 7), np.tile(np.array([w["ll"] for w in want]), (rep, 1)))
    rows = dict(zip("dWz", (d, W, z)))
    rows.update({k: g for k, g in zip(GRADS, grads) if k != "bc"})
    for k, x in rows.items():
        x = x.reshape((rep, 15) + tuple(x.shape[1:])).cpu().numpy()
        lo = 0
        for s, n in enumerate(l7):   # per distinct series: the criterion's floor is that series' largest entry
            if n:
                close(x[:, lo:lo + n], np.broadcast_to(want[s][k], (rep,) + want[s][k].shape))
            lo += n
    bc = grads[1].reshape(rep, 7, J).cpu().numpy()
    for s in range(7):
        close(bc[:, s], np.broadcast_to(want[s]["bc"], (rep, J)))


# ---- autograd -------------------------------------------------------------------------------------------------------------------
def test_autograd_function(oracle, packed):
    """packed.log_likelihood under torch.autograd.grad with random cotangents, one of them 0 and one series failed: the op's
    gradients scaled, zero for both; a shared c receives the batch sum."""
    import torch
    J, B = 5, 9
    ref = reference(oracle, J, shared=True)
    lengths = [150, 0, 13, 27, 150, 1, 14, 150, 2]
    pk, (a, U, V, y) = pack_rect(packed, ref["arrays"], lengths, [0] * B)
    a = a.clone(); a[int(pk.offsets[3]) + 4] = -3.0   # series 3 fails at its row 5
    cs, = dev(ref["c"])
    g = torch.from_numpy(np.random.default_rng(1).standard_normal(B)).cuda()
    g[6] = 0.0
    for c in (cs, cs[None].repeat(B, 1)):
        ll0, grads, flag = packed.loglik_grad(pk, c, a, U, V, y)
        assert flag.tolist() == [0, 0, 0, 5, 0, 0, 0, 0, 0] and ll0[3] == -float("inf")
        tl = pk.t.clone().requires_grad_()
        pk2 = packed.Packed(tl, lengths)
        leaves = [x.clone().requires_grad_() for x in (c, a, U, V, y)]
        ll = packed.log_likelihood(pk2, *leaves)
        assert torch.equal(ll, ll0)
        got = torch.autograd.grad(ll, [tl] + leaves, grad_outputs=g)
        dead = (g == 0) | (flag != 0)
        gr = torch.where(dead, torch.zeros_like(g), g)
        for k, x, w in zip(("bt", "bc", "ba", "bU", "bV", "by"), got, grads):
            s = gr if k == "bc" else gr[pk.seg]
            w = torch.nan_to_num(w, nan=0.0) * s.reshape((-1,) + (1,) * (w.dim() - 1))
            if k == "bc" and c.dim() == 1:
                w = w.sum(0)
            assert x.shape == w.shape and bool(torch.isfinite(x).all()), k
            close(x, w.cpu().numpy())
            if k != "bc":
                assert not bool(pk.unpack(x)[3].any()) and not bool(pk.unpack(x)[6].any()), k
        no_grad = packed.log_likelihood(pk, c, a, U, V, y)
        assert not no_grad.requires_grad and torch.equal(no_grad, ll0)


@pytest.mark.parametrize("kind", ("sum", "product"))
@pytest.mark.parametrize("per_series", (True, False))
def test_kernel_layer(packed, kind, per_series):
    """packed.log_likelihood_kernel against autograd.log_likelihood_kernel called once per series on that series alone:
    values and every parameter gradient, parameters (B,) and shared 0-d, with a jitter and a mean."""
    import torch
    from celerite2_amd import autograd as ag, terms

    lengths = [1, 17, 40, 150]
    B = len(lengths)
    t, _, _, _, _, y = problem(None, B, NMAX, 2)
    rng = np.random.default_rng(11)
    yerr = rng.uniform(0.3, 0.5, (B, NMAX))
    pk, (yd, ed) = pack_rect(packed, (t, y, yerr), lengths)
    base = dict(S0=1.2, w0=1.1, Q=2.5, a=0.8, c=0.3, jitter=0.15, mean=0.3)
    vals = {k: (v * (1.0 + 0.1 * rng.random(B)) if per_series else np.float64(v)) for k, v in base.items()}
    g = rng.standard_normal(B)

    def kernel(p):
        sho, real = terms.SHOTerm(S0=p["S0"], w0=p["w0"], Q=p["Q"], regime="under"), terms.RealTerm(a=p["a"], c=p["c"])
        return sho + real if kind == "sum" else sho * real

    P = {k: torch.tensor(v, dtype=torch.float64, device="cuda", requires_grad=True) for k, v in vals.items()}
    ll = packed.log_likelihood_kernel(kernel(P), pk, yd, yerr=ed, jitter=P["jitter"], mean=P["mean"])
    assert tuple(ll.shape) == (B,)
    got = torch.autograd.grad(ll, list(P.values()), grad_outputs=torch.from_numpy(g).cuda())
    want_ll, want_g = [], {k: [] for k in P}
    for b, n in enumerate(lengths):
        Pb = {k: torch.tensor(float(v[b]) if per_series else float(v), dtype=torch.float64, device="cuda", requires_grad=True)
              for k, v in vals.items()}
        tb, yb, eb = dev(t[b:b + 1, :n], y[b:b + 1, :n], yerr[b:b + 1, :n])
        lb = ag.log_likelihood_kernel(kernel(Pb), tb, yb, yerr=eb, jitter=Pb["jitter"], mean=Pb["mean"])
        gb = torch.autograd.grad(lb, list(Pb.values()), grad_outputs=torch.full((1,), g[b], dtype=torch.float64, device="cuda"))
        want_ll.append(float(lb.detach()[0]))
        for k, x in zip(Pb, gb):
            want_g[k].append(float(x))
    close(ll.detach(), np.array(want_ll))
    for k, x in zip(P, got):
        w = np.array(want_g[k])
        close(x.detach().reshape(-1), w if per_series else np.array([w.sum()]))
    # the diag form, and the refusals
    ll_d = packed.log_likelihood_kernel(kernel(P), pk, yd, diag=ed * ed, jitter=P["jitter"], mean=P["mean"])
    close(ll_d.detach(), np.array(want_ll))
    with pytest.raises(ValueError, match="exactly one"):
        packed.log_likelihood_kernel(kernel(P), pk, yd)
    with pytest.raises(ValueError, match="TermConvolution"):
        packed.log_likelihood_kernel(terms.TermConvolution(kernel(P), 0.02), pk, yd, yerr=ed)
    with pytest.raises(TypeError, match="no tensor parameter"):
        packed.log_likelihood_kernel(terms.RealTerm(a=0.8, c=0.3), pk, yd, yerr=ed)


# ---- capture ----------------------------------------------------------------------------------------------------------------------
def test_graph_capture(oracle, packed):
    """One loglik_grad call on caller-owned work and out captured in torch.cuda.graph: the replay gives the eager bits, also on
    new data."""
    import torch
    J = 8
    ref = reference(oracle, J)
    pk, (a, U, V, y) = pack_rect(packed, ref["arrays"], ref["lengths"][:65])
    c, = dev(ref["c"][:65])
    work = packed.workspace(pk, J)
    out = tuple(torch.empty_like(x) for x in packed.loglik_grad(pk, c, a, U, V, y)[1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        packed.loglik_grad(pk, c, a, U, V, y, work=work, out=out)   # (warm-up on a side stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                        # (two kernel nodes in sequence: no parallel branches)
        ll_g, out_g, flag_g = packed.loglik_grad(pk, c, a, U, V, y, work=work, out=out)
    for scale in (1.0, 1.25):
        y2 = y * scale
        ll_e, out_e, flag_e = packed.loglik_grad(pk, c, a, U, V, y2)
        y.copy_(y2)
        for x in out:
            x.fill_(float("nan"))
        work.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(ll_g, ll_e) and torch.equal(flag_g, flag_e)
        for x, xe in zip(out_g, out_e):
            assert torch.equal(x, xe)
        y.copy_(y2 / scale)
