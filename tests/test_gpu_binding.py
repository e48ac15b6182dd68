# -*- coding: utf-8 -*-
"""What the Python layer over the C-ABI (celerite2_amd/ops.py) promises about ARGUMENTS, op by op, pinned on the smallest
batch at which the dimensions differ (B = 2, N = 5, M = 3, J = nrhs = K = 2): a tensor with one dimension too long is
refused by name before anything is launched; the shared form (N,) / (J,) of t, c, ts, t1, t2, x, alpha, P gives the bits
of the same values expanded to (B, N) / (B, J) (a wrong batch stride or a swapped stride / pointer pair would not);
caller-owned outputs come back as the same objects with the same bits; an output that is an input is refused.  No
numerical accuracy is asserted here: the parity suites own that."""
import re

import pytest

pytestmark = pytest.mark.gpu

B, N, M, J, R, K = 2, 5, 3, 2, 2, 2   # R = nrhs
GRADS = "bt,bc,ba,bU,bV,by"
COEFS = "ar,cr,ac,bc,cc,dc"


class Case:
    """One op: `sig` = positional parameters | keyword parameters, `name(a,b)` for a parameter that takes a tuple; the
    names are those of the op's error messages (`err` where a message uses another one) and the keys of `vals`.
    exempt: the arguments whose shape DEFINES a dimension (at most one per dimension of the op).  scratch: not
    shape-checked (byte workspaces).  shared: given as (N,), also accepted as (B, N).  owned(result) -> the outputs to hand
    back, by name.  alias: (output, input) that must be refused."""

    def __init__(self, op, sig, vals, exempt=(), static=None, pre=None, err=None, scratch=(), shared=(), owned=None,
                 alias=None, id=None):
        self.op, self.vals, self.static = op, vals, dict(static or {})
        self.exempt = {exempt} if isinstance(exempt, str) else set(exempt)
        self.pre, self.err, self.scratch, self.shared, self.owned, self.alias = pre, dict(err or {}), set(scratch), shared, owned, alias
        self.id = id or op
        pos, _, kw = sig.partition("|")
        parse = lambda s: [(p, tuple(g.split(",")) if g else p) for p, g in re.findall(r"(\w+)(?:\(([\w,]+)\))?", s)]
        self.pos, self.kw = parse(pos), parse(kw)

    def call(self, ops, D, vals):
        pick = lambda names: tuple(vals[n] for n in names) if isinstance(names, tuple) else vals[names]
        have = lambda names: all(n in vals for n in (names if isinstance(names, tuple) else (names,)))
        args = ([self.pre(D)] if self.pre else []) + [pick(names) for _, names in self.pos]
        kw = {p: pick(names) for p, names in self.kw if have(names)}
        return getattr(ops, self.op)(*args, **kw, **self.static)


def zipped(names, tensors):
    return dict(zip(names.split(","), tensors))


SWEEP = dict(shared=("t", "c"), exempt=("U", "Y"))
TERMS = dict(vals=lambda D: dict(D, x=D["t"]), exempt=("diag", "ar", "ac"), shared=("x",))
EV = dict(vals=lambda D: dict(D, work=D["evwork"]), exempt=("U", "Us"), shared=("t", "ts", "c"))

CASES = [
    Case("factor", "t c a U V | d W S", lambda D: {k: D[k] for k in "tcaUV"}, exempt="U", static=dict(workspace=True), shared=("t", "c"),
         owned=lambda r: zipped("d,W,S", r)),
    Case("condition", "t c a U V", lambda D: D, exempt="U", shared=("t", "c")),
    Case("factor_rev", "t c a U V d W S bd bW", lambda D: D, exempt="U", shared=("t", "c")),
    Case("loglik", "t c a U V y", lambda D: D, exempt="U", shared=("t", "c")),
    Case("loglik_grad", "t c a U V y | work out(%s)" % GRADS, lambda D: dict(D, work=D["llwork"]), exempt="U", scratch=("work",),
         shared=("t", "c"), owned=lambda r: zipped(GRADS, r[1])),
    Case("dot_tril", "t c U W d Y | Z", lambda D: D, owned=lambda r: dict(Z=r), **SWEEP),
    Case("get_celerite_matrices", "ar ac bc dc x diag", **TERMS),
    Case("kernel_values", "ar cr ac bc cc dc t1 t2", lambda D: dict(D, t1=D["t"], t2=D["ts"]), exempt=("ar", "ac", "t1", "t2"),
         static=dict(B=B), shared=("t1", "t2")),
    Case("colsumsq_over_d", "Z d", lambda D: dict(D, Z=D["Y"]), exempt="Z"),
    Case("inverse_diag", "t c U W d z | q alpha", lambda D: D, exempt="U", shared=("t", "c"),
         owned=lambda r: zipped("q,alpha", r), alias=("q", "d")),
    Case("inverse_diag", "t c U W d z | q alpha ws(Mws,Fws)", lambda D: {k: v for k, v in D.items() if k not in ("Mws", "Fws")},
         exempt="U", static=dict(workspace=True), shared=("t", "c"), id="inverse_diag[workspace]",
         owned=lambda r: dict(q=r[0], alpha=r[1], Mws=r[2][0], Fws=r[2][1]), alias=("q", "d")),
    Case("inverse_diag_rev", "t c U W d z q alpha ws(Mws,Fws) bq balpha | out(bt,bc,bU,bW,bd,bz)",
         lambda D: dict(D, q=D["idq"], alpha=D["idalpha"]), exempt="U", shared=("t", "c"),
         owned=lambda r: zipped("bt,bc,bU,bW,bd,bz", r), alias=("bd", "d")),
    Case("get_celerite_matrices_rev", "ac bc dc x V bt bcv ba bU bV", lambda D: dict(D, x=D["t"], bt=D["bd"], bcv=D["bcv"], ba=D["bq"],
                                                                                     bU=D["bW"], bV=D["bW2"]),
         exempt=("V", "ac"), static=dict(Jr=0), err=dict(bcv="bc"), shared=("x",)),
    Case("explained_variance", "t ts c U W d Us Vs | out work", owned=lambda r: dict(out=r), alias=("work", "Us"), **EV),
    Case("explained_variance", "t ts c U W d Us Vs | out work ws(Sws,Rws)", id="explained_variance[workspace]",
         static=dict(workspace=True), owned=lambda r: dict(out=r[0], Sws=r[1][0], Rws=r[1][1]), alias=("work", "Us"),
         **dict(EV, vals=lambda D: {k: v for k, v in dict(D, work=D["evwork"]).items() if k not in ("Sws", "Rws")})),
    Case("explained_variance_rev", "t ts c U W d Us Vs work ws(Sws,Rws) br | out(bt,bts,bc,bU,bW,bd,bUs,bVs)",
         owned=lambda r: zipped("bt,bts,bc,bU,bW,bd,bUs,bVs", r), alias=("bUs", "Us"), **EV),
    Case("prior_draw", "t ts c U V Us Vs nt ns | ft fs", lambda D: D, exempt=("U", "Us", "nt"), shared=("t", "ts", "c"),
         owned=lambda r: zipped("ft,fs", r), alias=("ft", "V")),
    Case("loglik_terms", "ar cr ac bc cc dc x diag y | work", scratch=("work",),
         **dict(TERMS, vals=lambda D: dict(D, x=D["t"], work=D["ltwork"]))),
    Case("loglik_terms_grad", "ar cr ac bc cc dc x diag y | work out(bar,bcr,bac,bbc,bcc,bdc,bx,bdiag,by)", scratch=("work",),
         err={k: "out" for k in "bar,bcr,bac,bbc,bcc,bdc,bx,bdiag,by".split(",")},
         owned=lambda r: zipped("bar,bcr,bac,bbc,bcc,bdc,bx,bdiag,by", r[1]),
         **dict(TERMS, vals=lambda D: dict(D, x=D["t"], work=D["ltwork"]))),
    Case("term_coefficients", "P | out(%s)" % COEFS, lambda D: {"P": D["P"]}, pre=lambda D: D["program"], static=dict(B=B),
         shared=("P",), owned=lambda r: zipped(COEFS, r[0])),
    Case("term_coefficients", "P | out(%s) shift work" % COEFS, lambda D: {"P": D["Pe"], "work": D["exprwork"]},
         pre=lambda D: D["expr"], static=dict(B=B), scratch=("work",), shared=("P",), id="term_coefficients[expr]",
         owned=lambda r: dict(zipped(COEFS, r[0]), shift=r[2])),
    Case("term_coefficients_rev", "P cotangents(bar,bcr,bac,bbc,bcc,bdc) | out", lambda D: dict(D["cots"], P=D["P"]),
         pre=lambda D: D["program"], exempt=("bac",), err=dict(out="bP"), shared=("P",), owned=lambda r: dict(out=r)),
    Case("term_coefficients_rev", "P cotangents(bar,bcr,bac,bbc,bcc,bdc) | out bshift work",
         lambda D: dict(D["cots"], P=D["Pe"], bshift=D["mean"], work=D["exprwork"]), pre=lambda D: D["expr"], exempt=("bac",),
         err=dict(out="bP"), scratch=("work",), shared=("P",), id="term_coefficients_rev[expr]", owned=lambda r: dict(out=r)),
    Case("noise_mean_apply", "yerr jitter mean y | out(diag,r)", lambda D: {k: D[k] for k in ("yerr", "jitter", "mean", "y")},
         exempt="y", owned=lambda r: zipped("diag,r", r)),
    Case("noise_mean_rev", "jitter bdiag by | out(bjitter,bmean)", lambda D: dict(jitter=D["jitter"], bdiag=D["bd"], by=D["bq"]),
         exempt=("by",), owned=lambda r: zipped("bjitter,bmean", r)),
    Case("noise_mean_shift_apply", "yerr jitter mean shift y | out(diag,r)",
         lambda D: dict({k: D[k] for k in ("yerr", "jitter", "mean", "y")}, shift=D["mean"]), exempt="y",
         owned=lambda r: zipped("diag,r", r)),
    Case("noise_mean_shift_rev", "jitter bdiag by | out(bjitter,bmean,bshift)",
         lambda D: dict(jitter=D["jitter"], bdiag=D["bd"], by=D["bq"]), exempt=("by",), owned=lambda r: zipped("bjitter,bmean,bshift", r)),
    Case("loglik_kernel_grad", "P x yerr jitter mean y | work out(bP,bjitter,bmean,bx,bdiag,by)",
         lambda D: dict({k: D[k] for k in ("P", "yerr", "jitter", "mean", "y")}, x=D["t"], work=D["kgwork"]),
         pre=lambda D: D["program"], exempt="y", scratch=("work",), err=dict(bx="out", bdiag="out", by="out"), shared=("P", "x"),
         owned=lambda r: zipped("bP,bjitter,bmean,bx,bdiag,by", r[1])),
]
for name in ("solve_lower", "solve_upper", "matmul_lower", "matmul_upper"):
    second = "V" if name.startswith("matmul") else "W"
    CASES.append(Case(name, "t c U W Y | Z F", lambda D, second=second: dict(D, W=D[second]),
                      static=dict(workspace=True, zero_z=True), owned=lambda r: zipped("Z,F", r), **SWEEP))
    CASES.append(Case(name + "_rev", "t c U W Y Z F bZ",
                      lambda D, name=name, second=second: dict(D, W=D[second], Z=D["Z:" + name], F=D["F:" + name]), **SWEEP))
for name in ("general_matmul_lower", "general_matmul_upper"):
    general = dict(exempt=("U", "V", "Y"), shared=("t1", "t2", "c"))
    CASES.append(Case(name, "t1 t2 c U V Y | Z F", lambda D: dict(D, t1=D["t"], t2=D["ts"], V=D["Vs"], Y=D["Ym"]),
                      static=dict(workspace=True, zero_z=True), owned=lambda r: zipped("Z,F", r), **general))
    CASES.append(Case(name + "_rev", "t1 t2 c U V Y F bZ | out(bt1,bt2,bc,bU,bV,bY)",
                      lambda D, name=name: dict(D, t1=D["t"], t2=D["ts"], V=D["Vs"], Y=D["Ym"], F=D["F:" + name]),
                      owned=lambda r: zipped("bt1,bt2,bc,bU,bV,bY", r), alias=("bU", "U"), **general))
for name in ("kron_loglik", "kron_loglik_grad"):
    CASES.append(Case(name, "t c a U V alpha diag y", lambda D: dict(D, alpha=D["kalpha"], diag=D["kdiag"], y=D["ky"]), exempt=("U", "diag"),
                      shared=("t", "c", "alpha")))
IDS = [c.id for c in CASES]
NO_TENSORS = {"loglik_grad_workspace", "loglik_kernel_workspace", "TermProgram", "TermExpr"}


@pytest.fixture(scope="module")
def ops():
    import torch
    from celerite2_amd import ops as o
    assert torch.cuda.is_available()
    return o


@pytest.fixture(scope="module")
def D(ops):
    """Every input of every case, computed once: sorted times, one complex term (Jr = 0, Jc = 1, so J = 2), the positive
    definite matrix get_celerite_matrices makes of it, and what the forward ops return for it."""
    import torch
    g = torch.Generator().manual_seed(20)
    rand = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64).cuda()
    D = {}
    D["t"] = torch.cumsum(0.3 + rand(N), 0)
    D["ts"] = D["t"][0] + torch.cumsum(0.45 + rand(M), 0)
    D["ar"], D["cr"] = rand(0), rand(0)
    D["ac"], D["bc"], D["cc"], D["dc"] = (torch.tensor([v], dtype=torch.float64, device="cuda") for v in (1.0, 0.1, 0.5, 1.3))
    D["c"] = torch.cat([D["cc"], D["cc"]])
    D["diag"] = 0.1 + rand(B, N)
    D["a"], D["U"], D["V"] = ops.get_celerite_matrices(D["ar"], D["ac"], D["bc"], D["dc"], D["t"], D["diag"])
    _, D["Us"], D["Vs"] = ops.get_celerite_matrices(D["ar"], D["ac"], D["bc"], D["dc"], D["ts"], torch.zeros((B, M), dtype=torch.float64, device="cuda"))
    D["d"], D["W"], D["S"], flag = ops.factor(D["t"], D["c"], D["a"], D["U"], D["V"], workspace=True)
    assert int(flag.abs().sum()) == 0
    for k, shape in dict(y=(B, N), z=(B, N), bd=(B, N), bq=(B, N), balpha=(B, N), bW=(B, N, J), bW2=(B, N, J), bcv=(B, J),
                         Y=(B, N, R), bZ=(B, N, R), Ym=(B, M, R), br=(B, M), nt=(B, N, K), ns=(B, M, K), kdiag=(B, N, M),
                         ky=(B, N, M), kalpha=(M,), yerr=(B, N), jitter=(B,), mean=(B,)).items():
        D[k] = 0.5 + rand(*shape)
    for name in ("solve_lower", "solve_upper", "matmul_lower", "matmul_upper"):
        D["Z:" + name], D["F:" + name] = getattr(ops, name)(D["t"], D["c"], D["U"], D["V" if name.startswith("matmul") else "W"],
                                                            D["Y"], workspace=True, zero_z=True)
    for name in ("general_matmul_lower", "general_matmul_upper"):
        _, D["F:" + name] = getattr(ops, name)(D["t"], D["ts"], D["c"], D["U"], D["Vs"], D["Ym"], workspace=True)
    D["idq"], D["idalpha"], (D["Mws"], D["Fws"]) = ops.inverse_diag(D["t"], D["c"], D["U"], D["W"], D["d"], D["z"], workspace=True)
    D["evwork"] = torch.empty((B, M, J), dtype=torch.float64, device="cuda")
    _, (D["Sws"], D["Rws"]) = ops.explained_variance(D["t"], D["ts"], D["c"], D["U"], D["W"], D["d"], D["Us"], D["Vs"],
                                                     work=D["evwork"], workspace=True)
    D["llwork"] = ops.loglik_grad_workspace(B, N, J, "cuda")
    D["ltwork"] = ops.loglik_terms_workspace(B, N, 0, 1, "cuda")
    D["program"] = ops.TermProgram([dict(kind="complex", cols=(0, 1, 2, 3))], 4)
    D["expr"] = ops.TermExpr([dict(kind="complex", cols=(0, 1, 2, 3))], [dict(op="convolve", a=(0, 0, 0, 1), col=4)], 5)
    D["P"] = torch.tensor([1.0, 0.1, 0.5, 1.3], dtype=torch.float64, device="cuda")
    D["Pe"] = torch.tensor([1.0, 0.1, 0.5, 1.3, 0.2], dtype=torch.float64, device="cuda")
    D["exprwork"] = D["expr"].workspace(B, "cuda")
    D["kgwork"] = ops.loglik_kernel_workspace(D["program"], B, N, "cuda")
    D["cots"] = {k: 0.5 + rand(B, w) for k, w in zip(("bar", "bcr", "bac", "bbc", "bcc", "bdc"), (0, 0, 1, 1, 1, 1))}
    torch.cuda.synchronize()
    return D


def tensors(result):
    import torch
    if isinstance(result, torch.Tensor):
        return [result]
    if isinstance(result, (tuple, list)):
        return [x for r in result for x in tensors(r)]
    return []


def bits(x):
    import torch
    return x.clone() if x.dtype != torch.float64 else x.view(torch.int64).clone()


def same_bits(got, want):
    import torch
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert torch.equal(bits(g), w)


def test_every_op_has_a_case(ops):
    assert {c.op for c in CASES} == set(ops.__all__) - NO_TENSORS


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_one_dimension_too_long_is_refused_by_name(ops, D, case):
    """Inputs and caller-owned outputs alike, every dimension of every tensor in turn."""
    import torch
    vals = case.vals(D)
    if case.owned:
        vals = dict(vals, **case.owned(case.call(ops, D, vals)))
    names = [n for _, g in case.pos + case.kw for n in (g if isinstance(g, tuple) else (g,)) if n in vals]
    exempt = [n for n in names if n in case.exempt]
    assert len(exempt) == len(case.exempt) <= 4 and not case.exempt & case.scratch
    checked = 0
    for n in names:
        if n in case.exempt or n in case.scratch:
            continue
        for k in range(vals[n].dim()):
            shape = list(vals[n].shape)
            shape[k] += 1
            with pytest.raises(ValueError) as e:
                case.call(ops, D, dict(vals, **{n: torch.zeros(shape, dtype=torch.float64, device="cuda")}))
            assert str(e.value).startswith("Invalid shape: %s " % case.err.get(n, n)), (n, shape, str(e.value))
            checked += 1
    assert checked >= len(names) - len(exempt) - len(case.scratch)


@pytest.mark.parametrize("case", [c for c in CASES if c.shared], ids=[c.id for c in CASES if c.shared])
def test_shared_form_gives_the_bits_of_the_per_series_form(ops, D, case):
    vals = case.vals(D)
    want = [bits(x) for x in tensors(case.call(ops, D, vals))]
    assert want
    for n in case.shared:
        assert vals[n].dim() == 1
        expanded = vals[n].unsqueeze(0).expand(B, -1).contiguous()
        same_bits(tensors(case.call(ops, D, dict(vals, **{n: expanded}))), want)
    every = {n: vals[n].unsqueeze(0).expand(B, -1).contiguous() for n in case.shared}
    same_bits(tensors(case.call(ops, D, dict(vals, **every))), want)


@pytest.mark.parametrize("case", [c for c in CASES if c.owned], ids=[c.id for c in CASES if c.owned])
def test_caller_owned_outputs_come_back(ops, D, case):
    vals = case.vals(D)
    first = case.call(ops, D, vals)
    want = [bits(x) for x in tensors(first)]
    owned = case.owned(first)
    for x in owned.values():   # what the second call leaves untouched must not pass for written (zeros: what the general
        x.zero_()              # products allocate for F, whose start row they never write)
    second = tensors(case.call(ops, D, dict(vals, **owned)))
    for n, x in owned.items():
        assert any(x is y for y in second), n
    same_bits(second, want)
    if case.alias:
        out, inp = case.alias
        with pytest.raises(ValueError, match="must not alias"):
            case.call(ops, D, dict(vals, **dict(owned, **{out: vals[inp]})))
