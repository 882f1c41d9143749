"""GPU: the pullback of the solve (cnf_integrate_fixed_vjp / cnf_integrate_grid_vjp) and the autograd layer on top of it
(inference / generate with differentiable=True, a custom loss in ICNFModel.fit), against float64 autograd through
tests/vjp_reference.py.

Tolerance of every gradient: 5e-5 max|ref| + 1e-6, the bound the project uses for the same reverse sweeps
(test_parity_gpu.py: the parameter gradient against the fp64 oracle); forward values: 1e-4 absolute (TOL_SOLVE there)."""
import numpy as np
import pytest
import torch

import vjp_reference as ref

pytestmark = pytest.mark.gpu

ACTS = {0: "identity", 1: "tanh", 2: "softplus", 4: "sigmoid", 5: "swish", 6: "elu", 7: "gelu"}
TOL_SOLVE = 1e-4
LAM = (0.01, 0.02, 0.03)


def grad_close(got, want, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err, bound = np.abs(got - want).max(), 5e-5 * np.abs(want).max() + 1e-6
    print(f"{what}: err {err:.3e} bound {bound:.3e} (max|ref| {np.abs(want).max():.3e})")
    assert err <= bound, (what, err, bound)


def dev(a):
    return None if a is None else torch.tensor(np.asarray(a, dtype=np.float32), device="cuda:0")


def make_spec(o64, nvars, hidden, acts=1, **kw):
    s = o64.make_spec(nvars, hidden, **kw)
    if isinstance(acts, int):
        acts = [acts] * len(hidden)
    s.acts = list(acts) + [0] * (len(hidden) + 1 - len(acts))
    s.check()
    return s


def make_icnf(pkg, spec, alg, nsteps, lambdas=LAM, tspan=(0.0, 1.0), **kw):
    layers = [pkg.Dense(spec.widths[i], spec.widths[i + 1], ACTS[spec.acts[i]]) for i in range(len(spec.acts))]
    cm = (pkg.HIPJacVecMatrixMode if spec.mode == 1 else pkg.HIPVecJacMatrixMode)()
    return pkg.ICNF(nvariables=spec.nvars, naugments=spec.naug, nconditions=spec.ncond, autonomous=spec.autonomous,
                    nn=pkg.Chain(*layers), compute_mode=cm, steer_rate=0.0, tspan=tspan,
                    lambda1=lambdas[0] if spec.reg_z else 0.0, lambda2=lambdas[1] if spec.reg_j else 0.0,
                    lambda3=lambdas[2] if spec.reg_aug else 0.0, nprobes=spec.nprobes, device="cuda:0",
                    sol_kwargs=dict(alg=pkg.Tsit5() if alg == 1 else pkg.RK4(), adaptive=False, nsteps=nsteps), **kw)


def mode_of(pkg, spec):
    return pkg.TestMode() if spec.mode == 2 else pkg.TrainMode(bool(spec.reg_z or spec.reg_j or spec.reg_aug))


def inputs(o64, spec, B, seed):
    """Parameters, a full initial state (every row non-zero), probes, conditions and a Gaussian cotangent with every row non-zero."""
    p, xs, eps, ys = o64.synth_inputs(spec, B, seed, bias_scale=0.2)
    rng = np.random.default_rng(1000 + seed)
    u0 = np.concatenate([xs, 0.5 * rng.standard_normal((spec.naug + 3, B))], 0).astype(np.float32)
    bar = rng.standard_normal((spec.D + 3, B)).astype(np.float32)
    return p, u0, eps, ys, bar


def run_vjp(pkg, icnf, spec, p, u0, eps, ys, bar, t0=0.0, t1=1.0, tgrid=None):
    g, u0_bar, u1 = pkg.integrate_vjp(icnf, mode_of(pkg, spec), dev(u0), dev(p), dev(bar), t0=t0, t1=t1,
                                      eps=None if spec.mode == 2 else dev(eps), ys=dev(ys) if spec.ncond else None, tgrid=tgrid)
    return g.cpu().numpy(), u0_bar.cpu().numpy(), u1.cpu().numpy()


def check_pullback(pkg, o64, spec, alg, nsteps, B, path, seed=3, t0=0.0, t1=1.0, tgrid=None):
    p, u0, eps, ys, bar = inputs(o64, spec, B, seed)
    icnf = make_icnf(pkg, spec, alg, nsteps, tspan=(min(t0, t1), max(t0, t1)))
    assert pkg.vjp_path(icnf, mode_of(pkg, spec), B, alg, tgrid is not None) == path
    g, u0_bar, u1 = run_vjp(pkg, icnf, spec, p, u0, eps, ys, bar, t0, t1, tgrid)
    gr, ur, u1r = ref.pullback(o64, spec, p, u0, bar, t0, t1, nsteps, alg, eps, ys, tgrid)
    err = np.abs(u1 - u1r).max()
    print(f"u1: err {err:.3e}")
    assert err < TOL_SOLVE, err
    grad_close(g, gr, "grad")
    grad_close(u0_bar, ur, "u0_bar")
    D = spec.D
    assert np.array_equal(u0_bar[D:], bar[D:])      # the dlogp / E / n rows feed nothing: passed through bit for bit


# ---- 1. the fused per-wave sweep in its cotangent form ----
FUSED = {
    "cfg2 shape B=100 Tsit5": (dict(nvars=8, hidden=[64, 64, 64]), 1, 5, 100),
    "cfg2 shape B=37 RK4": (dict(nvars=8, hidden=[64, 64, 64]), 0, 6, 37),
    "cfg2 shape B=100 RK4": (dict(nvars=8, hidden=[64, 64, 64]), 0, 4, 100),
    "cfg2 shape B=37 Tsit5": (dict(nvars=8, hidden=[64, 64, 64]), 1, 3, 37),
    "cfg1 shape": (dict(nvars=2, hidden=[32, 32]), 1, 5, 33),
    "default net nvariables=1, reg_z reg_j": (dict(nvars=1, naug=2, hidden=[16, 16], acts=2, reg_z=True, reg_j=True, reg_aug=True), 1, 4, 50),
    "softplus two layers, naug": (dict(nvars=3, naug=2, hidden=[48, 48], acts=2, reg_z=True), 0, 4, 41),
    "conditioned RNODE": (dict(nvars=8, ncond=8, hidden=[64, 64, 64], reg_z=True, reg_j=True), 1, 3, 40),
}


@pytest.mark.parametrize("name", sorted(FUSED))
def test_fused_pullback_against_fp64(name, pkg, oracles):
    kw, alg, nsteps, B = FUSED[name]
    o64, _ = oracles
    kw = dict(kw)
    spec = make_spec(o64, kw.pop("nvars"), kw.pop("hidden"), kw.pop("acts", 1), **kw)
    check_pullback(pkg, o64, spec, alg, nsteps, B, path=1)


def test_fused_pullback_on_a_grid_and_backwards(pkg, oracles):
    o64, _ = oracles
    spec = make_spec(o64, 8, [64, 64, 64], 1, reg_z=True, reg_j=True)
    check_pullback(pkg, o64, spec, 1, 4, 45, path=1, tgrid=[0.0, 0.1, 0.35, 0.7, 1.0])
    check_pullback(pkg, o64, spec, 0, 3, 45, path=1, tgrid=[0.0, 0.5, 0.6, 1.0], seed=4)
    check_pullback(pkg, o64, spec, 1, 4, 45, path=1, t0=1.0, t1=0.0, seed=5)                       # generate's direction
    spec = make_spec(o64, 2, [32, 32], 2, naug=1)
    check_pullback(pkg, o64, spec, 1, 3, 20, path=1, tgrid=[1.0, 0.8, 0.3, 0.0], seed=6)           # a reversed grid


# ---- 2. the layer-wise sweep: everything else ----
LAYERED = {
    "JVP mode": (dict(nvars=3, hidden=[32, 32], acts=1, mode=1, reg_z=True, reg_j=True), 1, 3, 30),
    "JVP mode, two probes": (dict(nvars=3, hidden=[32, 32], acts=2, mode=1, nprobes=2), 0, 3, 21),
    "GELU / sigmoid chain": (dict(nvars=4, hidden=[32, 48], acts=[7, 4], reg_z=True, reg_j=True), 1, 3, 25),
    "swish / ELU chain, conditioned": (dict(nvars=3, ncond=2, hidden=[24, 24, 24], acts=[5, 6, 5]), 0, 3, 19),
    "K = 4 probes": (dict(nvars=8, hidden=[64, 64, 64], acts=1, nprobes=4, reg_z=True, reg_j=True), 1, 3, 24),
    "exact trace": (dict(nvars=4, hidden=[32, 32], acts=1, mode=2), 1, 3, 18),
    "32 / 3x256 (cooperative shape)": (dict(nvars=32, hidden=[256, 256, 256], acts=1), 0, 2, 24),
    "default architecture nvariables=8 (slab shape)": (dict(nvars=8, naug=9, hidden=[72, 72], acts=2, reg_z=True, reg_j=True, reg_aug=True), 1, 2, 20),
    "default architecture nvariables=20 (dealt cooperative shape)": (dict(nvars=20, naug=21, hidden=[168, 168], acts=2), 0, 2, 16),
    "small B": (dict(nvars=12, hidden=[48, 48, 48, 48], acts=1, reg_z=True), 1, 3, 3),
}


@pytest.mark.parametrize("name", sorted(LAYERED))
def test_layerwise_pullback_against_fp64(name, pkg, oracles):
    kw, alg, nsteps, B = LAYERED[name]
    o64, _ = oracles
    kw = dict(kw)
    spec = make_spec(o64, kw.pop("nvars"), kw.pop("hidden"), kw.pop("acts", 1), **kw)
    check_pullback(pkg, o64, spec, alg, nsteps, B, path=2)


def test_layerwise_pullback_on_a_grid(pkg, oracles):
    o64, _ = oracles
    spec = make_spec(o64, 4, [32, 48], [7, 4], reg_z=True, reg_j=True)
    check_pullback(pkg, o64, spec, 1, 3, 22, path=2, tgrid=[0.0, 0.2, 0.45, 1.0])


def test_unsupported_width_reports_no_path(pkg, oracles):
    o64, _ = oracles
    spec = make_spec(o64, 4, [700, 700], 1)
    icnf = make_icnf(pkg, spec, 1, 2)
    assert pkg.vjp_path(icnf, pkg.TrainMode(False), 8) == 0
    p, u0, eps, ys, bar = inputs(o64, spec, 8, 2)
    with pytest.raises(pkg._lib.CnfError) as e:
        run_vjp(pkg, icnf, spec, p, u0, eps, ys, bar)
    assert e.value.code == pkg._lib.ERR_UNSUPPORTED


# ---- 3. the shipped gradient is this pullback with one particular cotangent (no oracle involved) ----
@pytest.mark.parametrize("kw,alg,nsteps,B,path", [
    (dict(nvars=3, naug=2, hidden=[32, 32], acts=2, reg_z=True, reg_j=True, reg_aug=True), 1, 5, 70, 1),
    (dict(nvars=4, hidden=[32, 48], acts=[7, 4], reg_z=True, reg_j=True), 0, 4, 40, 2),
])
def test_identity_with_the_shipped_gradient(kw, alg, nsteps, B, path, pkg, oracles):
    o64, _ = oracles
    kw = dict(kw)
    spec = make_spec(o64, kw.pop("nvars"), kw.pop("hidden"), kw.pop("acts", 1), **kw)
    p, xs, eps, ys = o64.synth_inputs(spec, B, 8, bias_scale=0.2)
    icnf = make_icnf(pkg, spec, alg, nsteps)
    m = mode_of(pkg, spec)
    assert pkg.vjp_path(icnf, m, B, alg) == path
    L, g, gx = pkg.loss_and_gradient(icnf, m, dev(xs), dev(p), {}, eps=dev(eps), wrt_x=True)
    u0 = np.concatenate([xs, np.zeros((spec.naug + 3, B), np.float32)], 0)
    zero = np.zeros_like(u0)
    _, _, u1 = run_vjp(pkg, icnf, spec, p, u0, eps, ys, zero)                                   # the call's own u1
    lam = (icnf.lambda1, icnf.lambda2, icnf.lambda3)
    bar = ref.loss_cotangent(spec, u1, lam, B)
    g2, u0_bar, _ = run_vjp(pkg, icnf, spec, p, u0, eps, ys, bar)
    grad_close(g2, g.cpu().numpy(), "grad vs cnf_loss_grad_fixed")
    grad_close(u0_bar[:spec.nvars], gx.cpu().numpy(), "u0_bar vs grad_x")


# ---- 4. columns are independent ----
@pytest.mark.parametrize("kw,path", [(dict(nvars=8, hidden=[64, 64, 64], acts=1, reg_z=True, reg_j=True), 1),
                                     (dict(nvars=4, hidden=[32, 48], acts=[7, 4], reg_z=True, reg_j=True), 2)])
def test_columns_are_independent(kw, path, pkg, oracles):
    o64, _ = oracles
    kw = dict(kw)
    spec = make_spec(o64, kw.pop("nvars"), kw.pop("hidden"), kw.pop("acts", 1), **kw)
    B = 48
    p, u0, eps, ys, bar = inputs(o64, spec, B, 12)
    icnf = make_icnf(pkg, spec, 1, 4)
    assert pkg.vjp_path(icnf, mode_of(pkg, spec), B, 1) == path
    g, u0_bar, u1 = run_vjp(pkg, icnf, spec, p, u0, eps, ys, bar)
    assert np.array_equal(u0_bar[spec.D:], bar[spec.D:])
    # zero cotangent columns give zero u0_bar columns
    bz = bar.copy()
    bz[:, 5:20] = 0.0
    _, uz, _ = run_vjp(pkg, icnf, spec, p, u0, eps, ys, bz)
    assert np.all(uz[:, 5:20] == 0.0)
    assert np.array_equal(uz[:, 20:], u0_bar[:, 20:]) and np.array_equal(uz[:, :5], u0_bar[:, :5])
    # the grad of B columns is the sum of the grads of two halves (different summation order: the gradient tolerance, against the
    # float64 sum of the halves)
    ga, ua, _ = run_vjp(pkg, icnf, spec, p, u0[:, :32], eps[:, :32], ys, bar[:, :32])
    gb, ub, _ = run_vjp(pkg, icnf, spec, p, u0[:, 32:], eps[:, 32:], ys, bar[:, 32:])
    grad_close(g, ga.astype(np.float64) + gb.astype(np.float64), "grad = sum of halves")
    # (calls of different sizes may take different forward kernels and product tilings: the gradient tolerance, not bits)
    grad_close(np.concatenate([ua, ub], 1), u0_bar, "u0_bar of the halves")
    # a ragged last tile leaks nothing: B = 37 is the first 37 columns of B = 48
    g37, u37, u1_37 = run_vjp(pkg, icnf, spec, p, u0[:, :37], eps[:, :37], ys, bar[:, :37])
    grad_close(u37, u0_bar[:, :37], "u0_bar of 37 columns")
    assert np.abs(u1_37 - u1[:, :37]).max() < TOL_SOLVE
    b37 = bar.copy()
    b37[:, 37:] = 0.0
    g48, _, _ = run_vjp(pkg, icnf, spec, p, u0, eps, ys, b37)
    grad_close(g37, g48, "grad of 37 columns = grad of 48 with 11 zero cotangents")
    # B = 0 zeroes grad
    g0, _, _ = run_vjp(pkg, icnf, spec, p, u0[:, :0], eps[:, :0], ys, bar[:, :0])
    assert g0.shape == g.shape and np.all(g0 == 0.0)


# ---- 5. autograd on top ----
def _ref_inference(o64, spec, pt, xt, nsteps, alg, eps, ys=None, basedist=None):
    """float64: (logp, E, n, A) of the columns of xt through vjp_reference.integrate, with a graph to pt and xt."""
    D, B = spec.D, xt.shape[1]
    u0 = torch.cat([xt, torch.zeros(spec.naug + 3, B, dtype=torch.float64)], 0)
    u1 = ref.integrate(o64, spec, pt, u0, 0.0, 1.0, nsteps, alg, eps, ys)
    z = u1[:D]
    lp = (basedist.log_prob(z.t()) if basedist is not None else ref.std_normal_logpdf(z)) - u1[D]
    A = torch.sqrt((z[spec.nvars:] ** 2).sum(0)) if (spec.reg_aug and spec.naug > 0) else torch.zeros(B, dtype=torch.float64)
    return lp, u1[D + 1], u1[D + 2], A


@pytest.mark.parametrize("kw,path", [(dict(nvars=3, hidden=[32, 32], acts=1), 1), (dict(nvars=3, hidden=[32, 32], acts=7), 2)])
def test_autograd_weighted_nll_and_logsumexp(kw, path, pkg, oracles):
    o64, _ = oracles
    kw = dict(kw)
    spec = make_spec(o64, kw.pop("nvars"), kw.pop("hidden"), kw.pop("acts", 1), **kw)
    B, nsteps, alg = 40, 4, 1
    p, xs, eps, _ = o64.synth_inputs(spec, B, 21, bias_scale=0.2)
    p2 = o64.synth_inputs(spec, B, 22, bias_scale=0.2)[0]
    w = np.random.default_rng(3).uniform(0.2, 2.0, B)
    icnf = make_icnf(pkg, spec, alg, nsteps)
    m = pkg.TrainMode(False)
    assert pkg.vjp_path(icnf, m, B, alg) == path
    # (a) per-sample-weighted NLL
    ps, x = dev(p).requires_grad_(), dev(xs).requires_grad_()
    lp = pkg.inference(icnf, m, x, ps, {}, eps=dev(eps), differentiable=True)[0]
    plain = pkg.inference(icnf, m, dev(xs), dev(p), {}, eps=dev(eps))[0]
    assert lp.requires_grad and not plain.requires_grad
    assert float((lp.detach() - plain).abs().max()) < TOL_SOLVE
    L = -(dev(w) * lp).sum() / B
    gp, gx = torch.autograd.grad(L, (ps, x))
    pt, xt = ref.leaf(p), ref.leaf(xs)
    Lr = -(torch.tensor(w) * _ref_inference(o64, spec, pt, xt, nsteps, alg, eps)[0]).sum() / B
    rp, rx = torch.autograd.grad(Lr, (pt, xt))
    assert abs(float(L.detach()) - float(Lr.detach())) < TOL_SOLVE
    grad_close(gp.cpu().numpy(), rp.numpy(), "weighted NLL: ps")
    grad_close(gx.cpu().numpy(), rx.numpy(), "weighted NLL: xs")
    # (b) -logsumexp over two flows that share xs
    ps1, ps2, x = dev(p).requires_grad_(), dev(p2).requires_grad_(), dev(xs).requires_grad_()
    l1 = pkg.inference(icnf, m, x, ps1, {}, eps=dev(eps), differentiable=True)[0]
    l2 = pkg.inference(icnf, m, x, ps2, {}, eps=dev(eps), differentiable=True)[0]
    L = -torch.logsumexp(torch.stack([l1, l2]), 0).mean()
    g1, g2, gx = torch.autograd.grad(L, (ps1, ps2, x))
    pt1, pt2, xt = ref.leaf(p), ref.leaf(p2), ref.leaf(xs)
    r1 = _ref_inference(o64, spec, pt1, xt, nsteps, alg, eps)[0]
    r2 = _ref_inference(o64, spec, pt2, xt, nsteps, alg, eps)[0]
    Lr = -torch.logsumexp(torch.stack([r1, r2]), 0).mean()
    q1, q2, qx = torch.autograd.grad(Lr, (pt1, pt2, xt))
    assert abs(float(L.detach()) - float(Lr.detach())) < TOL_SOLVE
    grad_close(g1.cpu().numpy(), q1.numpy(), "logsumexp: ps of flow 1")
    grad_close(g2.cpu().numpy(), q2.numpy(), "logsumexp: ps of flow 2")
    grad_close(gx.cpu().numpy(), qx.numpy(), "logsumexp: xs")


def test_autograd_under_a_custom_base_distribution(pkg, oracles):
    o64, _ = oracles
    spec = make_spec(o64, 3, [32, 32], 1)
    B, nsteps, alg = 50, 6, 1
    p, xs, eps, _ = o64.synth_inputs(spec, B, 4, bias_scale=0.2)
    icnf = make_icnf(pkg, spec, alg, nsteps)
    loc, var = [0.5, -1.0, 2.0], [0.25, 1.0, 4.0]
    icnf.basedist = torch.distributions.MultivariateNormal(torch.tensor(loc, device="cuda:0"),
                                                           covariance_matrix=torch.diag(torch.tensor(var, device="cuda:0")))
    m = pkg.TrainMode(False)
    with pytest.raises(NotImplementedError):        # the refusal of the fused functional stands
        pkg.loss_and_gradient(icnf, m, dev(xs), dev(p), {}, eps=dev(eps))
    ps, x = dev(p).requires_grad_(), dev(xs).requires_grad_()
    L = -pkg.inference(icnf, m, x, ps, {}, eps=dev(eps), differentiable=True)[0].mean()
    gp, gx = torch.autograd.grad(L, (ps, x))
    base64 = torch.distributions.MultivariateNormal(torch.tensor(loc, dtype=torch.float64),
                                                    covariance_matrix=torch.diag(torch.tensor(var, dtype=torch.float64)))
    pt, xt = ref.leaf(p), ref.leaf(xs)
    Lr = -_ref_inference(o64, spec, pt, xt, nsteps, alg, eps, basedist=base64)[0].mean()
    rp, rx = torch.autograd.grad(Lr, (pt, xt))
    assert abs(float(L.detach()) - float(Lr.detach())) < TOL_SOLVE
    grad_close(gp.cpu().numpy(), rp.numpy(), "custom base: ps")
    grad_close(gx.cpu().numpy(), rx.numpy(), "custom base: xs")


def test_autograd_through_generate(pkg, oracles):
    o64, _ = oracles
    spec = make_spec(o64, 3, [32, 32], 2, naug=1)
    n, nsteps, alg = 36, 5, 1
    p, _, eps, _ = o64.synth_inputs(spec, n, 9, bias_scale=0.2)
    z0 = np.random.default_rng(2).standard_normal((spec.D, n)).astype(np.float32)
    icnf = make_icnf(pkg, spec, alg, nsteps)
    m = pkg.TrainMode(False)
    ps, z = dev(p).requires_grad_(), dev(z0).requires_grad_()
    x = pkg.generate(icnf, m, ps, {}, n, z0=z, eps=dev(eps), differentiable=True)
    plain = pkg.generate(icnf, m, dev(p), {}, n, z0=dev(z0), eps=dev(eps))
    assert x.shape == (spec.nvars, n) and float((x.detach() - plain).abs().max()) < TOL_SOLVE
    L = (x * x).sum(0).mean()
    gp, gz = torch.autograd.grad(L, (ps, z))
    pt, zt = ref.leaf(p), ref.leaf(z0)
    u0 = torch.cat([zt, torch.zeros(3, n, dtype=torch.float64)], 0)
    xr = ref.integrate(o64, spec, pt, u0, 1.0, 0.0, nsteps, alg, eps)[:spec.nvars]
    Lr = (xr * xr).sum(0).mean()
    rp, rz = torch.autograd.grad(Lr, (pt, zt))
    assert abs(float(L.detach()) - float(Lr.detach())) < TOL_SOLVE
    grad_close(gp.cpu().numpy(), rp.numpy(), "generate: ps")
    grad_close(gz.cpu().numpy(), rz.numpy(), "generate: z0")


@pytest.mark.parametrize("kw,alg", [(dict(nvars=3, naug=2, hidden=[32, 32], acts=2, reg_z=True, reg_j=True, reg_aug=True), 1),
                                    (dict(nvars=4, hidden=[32, 48], acts=[7, 4], reg_z=True, reg_j=True), 0)])
def test_differentiable_inference_reproduces_loss_and_gradient(kw, alg, pkg, oracles):
    o64, _ = oracles
    kw = dict(kw)
    spec = make_spec(o64, kw.pop("nvars"), kw.pop("hidden"), kw.pop("acts", 1), **kw)
    B, nsteps = 60, 5
    p, xs, eps, _ = o64.synth_inputs(spec, B, 14, bias_scale=0.2)
    icnf = make_icnf(pkg, spec, alg, nsteps)
    m = mode_of(pkg, spec)
    Lw, gw, gxw = pkg.loss_and_gradient(icnf, m, dev(xs), dev(p), {}, eps=dev(eps), wrt_x=True)
    ps, x = dev(p).requires_grad_(), dev(xs).requires_grad_()
    lp, (E, nn, A) = pkg.inference(icnf, m, x, ps, {}, eps=dev(eps), differentiable=True)
    L = (-lp + icnf.lambda1 * E + icnf.lambda2 * nn + icnf.lambda3 * A).mean()
    gp, gx = torch.autograd.grad(L, (ps, x))
    assert abs(float(L.detach()) - float(Lw)) < TOL_SOLVE
    grad_close(gp.cpu().numpy(), gw.cpu().numpy(), "ps")
    grad_close(gx.cpu().numpy(), gxw.cpu().numpy(), "xs")


def test_differentiable_inference_under_adaptive_tsit5(pkg, oracles):
    """The backward runs on the grid the forward accepted (last_solve_stats), as loss_and_gradient does."""
    o64, _ = oracles
    spec = make_spec(o64, 3, [32, 32], 1)
    B = 32
    p, xs, eps, _ = o64.synth_inputs(spec, B, 17, bias_scale=0.2)
    icnf = make_icnf(pkg, spec, 1, 4)
    icnf.sol_kwargs = dict(alg=pkg.Tsit5(), abstol=1e-5, reltol=1e-5)
    assert icnf.adaptive
    m = pkg.TrainMode(False)
    ps, x = dev(p).requires_grad_(), dev(xs).requires_grad_()
    lp = pkg.inference(icnf, m, x, ps, {}, eps=dev(eps), differentiable=True)[0]
    grid = list(icnf.last_solve_stats["tgrid"])
    assert len(grid) >= 3 and grid[0] == 0.0 and grid[-1] == 1.0
    gp, gx = torch.autograd.grad(-lp.mean(), (ps, x))
    pt, xt = ref.leaf(p), ref.leaf(xs)
    u0 = torch.cat([xt, torch.zeros(3, B, dtype=torch.float64)], 0)
    u1 = ref.integrate(o64, spec, pt, u0, 0.0, 1.0, None, 1, eps, None, tgrid=grid)
    Lr = -(ref.std_normal_logpdf(u1[:3]) - u1[3]).mean()
    rp, rx = torch.autograd.grad(Lr, (pt, xt))
    grad_close(gp.cpu().numpy(), rp.numpy(), "adaptive: ps")
    grad_close(gx.cpu().numpy(), rx.numpy(), "adaptive: xs")


# ---- 6. a custom loss in ICNFModel.fit ----
def test_fit_with_a_custom_loss(pkg, oracles):
    """A custom loss with the package loss's value: two optimiser steps give the parameters of the default fit from the same
    generators.  As in test_mlj_model_fit_steps_and_transform_against_the_oracle the 2e-6 is asked where Adam's update is not
    the sign of rounding noise (|g| > 1e-3 max|g| in both steps, by the fp64 oracle's gradient); the rest moves by at most one
    step per epoch."""
    o64, _ = oracles
    n, nvars, naug, nsteps = 48, 2, 1, 6
    rng = np.random.default_rng(77)
    X = rng.standard_normal((n, nvars)).astype(np.float32) * 0.7 + 0.3
    probes = [rng.standard_normal((nvars + naug, n)).astype(np.float32) for _ in range(2)]
    lam = (0.01, 0.02, 0.03)
    eta, wd = 2e-3, 1e-4
    spec = make_spec(o64, nvars, [24, 24], 2, naug=naug, reg_z=True, reg_j=True, reg_aug=True)

    def fit(loss):
        calls = []

        def epsdist(gen, shape, device):
            k = len(calls)
            calls.append(shape)
            return torch.tensor(np.ascontiguousarray(probes[k].T), device=device)

        icnf = make_icnf(pkg, spec, 1, nsteps, lambdas=lam, epsdist=epsdist)
        model = pkg.ICNFModel(icnf=icnf, loss=loss, batchsize=0, epochs=2, eta=eta, weight_decay=wd, callback=None,
                              shuffle_rng=torch.Generator().manual_seed(4), init_rng=torch.Generator().manual_seed(5))
        (ps_fit, st), _, report = model.fit(X)
        assert report["stats"]["iterations"] == 2 and len(calls) == 2
        return icnf, ps_fit.cpu().numpy().astype(np.float64), report["stats"]["final_loss"]

    def custom(icnf, mode, xs, ps, st):
        lp, (E, nn, A) = pkg.inference(icnf, mode, xs, ps, st, differentiable=True)
        return (-lp + icnf.lambda1 * E + icnf.lambda2 * nn + icnf.lambda3 * A).mean()

    icnf, want, Lw = fit(None)
    _, got, Lg = fit(custom)
    # where the updates are not the sign of rounding noise: the oracle's gradients along the default fit's two steps
    p = pkg.setup(torch.Generator().manual_seed(5), icnf)[0].numpy().astype(np.float64)
    g_sh = torch.Generator().manual_seed(4)
    mm, vv, sens = np.zeros_like(p), np.zeros_like(p), []
    for k in range(2):
        idx = torch.randperm(n, generator=g_sh).numpy()
        _, g = o64.loss_and_grad(spec, p.astype(np.float32), X.T[:, idx], 0.0, 1.0, nsteps, 1, probes[k], None, lam)
        g = g + wd * p
        mm = 0.9 * mm + 0.1 * g
        vv = 0.999 * vv + 0.001 * g * g
        sens.append(np.abs(g) > 1e-3 * np.abs(g).max())
        p = p - eta * (mm / (1 - 0.9 ** (k + 1))) / (np.sqrt(vv / (1 - 0.999 ** (k + 1))) + 1e-8)
    ok = sens[0] & sens[1]
    assert ok.mean() > 0.8
    err = np.abs(got[ok] - want[ok]).max()
    print(f"custom fit vs default fit: {err:.3e}; final loss {Lg} vs {Lw}")
    assert err < 2e-6, err
    assert np.abs(got - want).max() <= 2.001 * 2 * eta
    assert abs(Lg - Lw) < TOL_SOLVE

    def no_graph(icnf, mode, xs, ps, st):
        return pkg.inference(icnf, mode, xs, ps, st)[0].mean()

    with pytest.raises(TypeError, match="differentiable=True"):
        fit(no_graph)
