"""GPU: the cotangent of the conditions of a conditioned flow (cnf_integrate_fixed_vjp_cond / cnf_integrate_grid_vjp_cond) and the
autograd layer on top of it (inference / generate with differentiable=True, cond_grad=True), against float64 autograd through
tests/cond_vjp_reference.py.

Tolerance of every cotangent: 5e-5 max|ref| + 1e-6; forward values: 1e-4 absolute - the bounds of test_vjp_gpu.py for the same
reverse sweeps."""
import numpy as np
import pytest
import torch

import cond_vjp_reference as cref

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


def spec_of(o64, kw):
    kw = dict(kw)
    return make_spec(o64, kw.pop("nvars"), kw.pop("hidden"), kw.pop("acts", 1), **kw)


def make_icnf(pkg, spec, alg, nsteps, tspan=(0.0, 1.0)):
    layers = [pkg.Dense(spec.widths[i], spec.widths[i + 1], ACTS[spec.acts[i]]) for i in range(len(spec.acts))]
    cm = (pkg.HIPJacVecMatrixMode if spec.mode == 1 else pkg.HIPVecJacMatrixMode)()
    return pkg.ICNF(nvariables=spec.nvars, naugments=spec.naug, nconditions=spec.ncond, autonomous=spec.autonomous,
                    nn=pkg.Chain(*layers), compute_mode=cm, steer_rate=0.0, tspan=tspan,
                    lambda1=LAM[0] if spec.reg_z else 0.0, lambda2=LAM[1] if spec.reg_j else 0.0,
                    lambda3=LAM[2] if spec.reg_aug else 0.0, nprobes=spec.nprobes, device="cuda:0",
                    sol_kwargs=dict(alg=pkg.Tsit5() if alg == 1 else pkg.RK4(), adaptive=False, nsteps=nsteps))


def mode_of(pkg, spec):
    return pkg.TestMode() if spec.mode == 2 else pkg.TrainMode(bool(spec.reg_z or spec.reg_j or spec.reg_aug))


def inputs(o64, spec, B, seed):
    """Parameters, a full initial state (every row non-zero), probes, conditions and a Gaussian cotangent with every row non-zero."""
    p, xs, eps, ys = o64.synth_inputs(spec, B, seed, bias_scale=0.2)
    rng = np.random.default_rng(1000 + seed)
    u0 = np.concatenate([xs, 0.5 * rng.standard_normal((spec.naug + 3, B))], 0).astype(np.float32)
    bar = rng.standard_normal((spec.D + 3, B)).astype(np.float32)
    return p, u0, eps, ys, bar


def run_cond(pkg, icnf, spec, p, u0, eps, ys, bar, t0=0.0, t1=1.0, tgrid=None):
    g, u0_bar, ys_bar, u1 = pkg.integrate_vjp(icnf, mode_of(pkg, spec), dev(u0), dev(p), dev(bar), t0=t0, t1=t1,
                                              eps=None if spec.mode == 2 else dev(eps), ys=dev(ys), tgrid=tgrid, want_ys_bar=True)
    assert ys_bar.shape == (spec.ncond, u0.shape[1])
    return g.cpu().numpy(), u0_bar.cpu().numpy(), ys_bar.cpu().numpy(), u1.cpu().numpy()


def check_cond_pullback(pkg, o64, spec, alg, nsteps, B, path, seed=3, t0=0.0, t1=1.0, tgrid=None):
    p, u0, eps, ys, bar = inputs(o64, spec, B, seed)
    icnf = make_icnf(pkg, spec, alg, nsteps, tspan=(min(t0, t1), max(t0, t1)))
    assert pkg.vjp_path(icnf, mode_of(pkg, spec), B, alg, tgrid is not None) == path
    g, u0_bar, ys_bar, u1 = run_cond(pkg, icnf, spec, p, u0, eps, ys, bar, t0, t1, tgrid)
    gr, ur, yr, u1r = cref.pullback(o64, spec, p, u0, ys, bar, t0, t1, nsteps, alg, eps, tgrid)
    err = np.abs(u1 - u1r).max()
    print(f"u1: err {err:.3e}")
    assert err < TOL_SOLVE, err
    grad_close(ys_bar, yr, "ys_bar")
    grad_close(g, gr, "grad")
    grad_close(u0_bar, ur, "u0_bar")


# ---- 1. the fused per-wave sweep (cnf_grad2_coty.hip) ----
FUSED = {
    "8 / 8 / 3x64 tanh, reg_z reg_j, two full tiles and a partial one": (dict(nvars=8, ncond=8, hidden=[64, 64, 64], reg_z=True, reg_j=True), 1, 3, 40),
    "3 conditions (no multiple of 4), softplus": (dict(nvars=2, ncond=3, hidden=[32, 32], acts=2), 0, 4, 33),
    "16 conditions": (dict(nvars=4, ncond=16, hidden=[48, 48, 48]), 1, 2, 21),
    "one hidden tile, two layers": (dict(nvars=2, ncond=1, hidden=[16, 16]), 1, 3, 5),
    "one hidden tile, three layers": (dict(nvars=2, ncond=1, hidden=[16, 16, 16]), 1, 3, 5),
    "ZR = 4": (dict(nvars=12, ncond=4, hidden=[64, 64]), 0, 3, 18),
}


@pytest.mark.parametrize("name", sorted(FUSED))
def test_fused_ys_bar_against_fp64(name, pkg, oracles):
    kw, alg, nsteps, B = FUSED[name]
    o64, _ = oracles
    check_cond_pullback(pkg, o64, spec_of(o64, kw), alg, nsteps, B, path=1)


def test_fused_ys_bar_on_a_grid_and_backwards(pkg, oracles):
    o64, _ = oracles
    spec = make_spec(o64, 8, [64, 64, 64], 1, ncond=8, reg_z=True, reg_j=True)
    check_cond_pullback(pkg, o64, spec, 1, 4, 40, path=1, tgrid=[0.0, 0.1, 0.35, 0.7, 1.0])
    check_cond_pullback(pkg, o64, spec, 0, 3, 40, path=1, tgrid=[1.0, 0.8, 0.3, 0.0], seed=4)     # a reversed grid
    check_cond_pullback(pkg, o64, spec, 1, 3, 40, path=1, t0=1.0, t1=0.0, seed=5)                 # generate's direction


def test_fused_ys_bar_where_a_wave_walks_a_second_tile(pkg, oracles):
    """More 16-sample tiles than the launch has waves (4 per compute unit): the waves of the first blocks take a second tile, whose
    sum over the stages must start from zero again."""
    o64, _ = oracles
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    spec = make_spec(o64, 2, [16, 16], 1, ncond=1)
    check_cond_pullback(pkg, o64, spec, 0, 2, 64 * cus + 19, path=1, seed=6)


# ---- 2. the layer-wise sweep: everything else ----
LAYERED = {
    "JVP mode, reg_z reg_j": (dict(nvars=3, ncond=2, hidden=[32, 32], acts=1, mode=1, reg_z=True, reg_j=True), 1, 3, 30),
    "JVP mode, two probes": (dict(nvars=3, ncond=3, hidden=[32, 32], acts=2, mode=1, nprobes=2), 0, 3, 21),
    "K = 4 probes, VJP mode": (dict(nvars=8, ncond=8, hidden=[64, 64, 64], acts=1, nprobes=4, reg_z=True, reg_j=True), 1, 3, 24),
    "exact trace": (dict(nvars=4, ncond=2, hidden=[32, 32], acts=1, mode=2), 1, 3, 18),
    "swish / ELU chain": (dict(nvars=3, ncond=2, hidden=[24, 24, 24], acts=[5, 6, 5]), 0, 3, 19),
    "GELU / sigmoid chain, autonomous": (dict(nvars=4, ncond=3, hidden=[32, 48], acts=[7, 4], autonomous=True, reg_z=True, reg_j=True), 1, 3, 25),
    "8 / 8 / 3x128 (cooperative shape)": (dict(nvars=8, ncond=8, hidden=[128, 128, 128], acts=1), 0, 2, 24),
    "default architecture nvariables=8, 2 conditions (slab shape)": (dict(nvars=8, naug=9, ncond=2, hidden=[72, 72], acts=2, reg_z=True, reg_j=True, reg_aug=True), 1, 2, 20),
    "small B": (dict(nvars=12, ncond=4, hidden=[48, 48, 48, 48], acts=1, reg_z=True), 1, 3, 3),
}


@pytest.mark.parametrize("name", sorted(LAYERED))
def test_layerwise_ys_bar_against_fp64(name, pkg, oracles):
    kw, alg, nsteps, B = LAYERED[name]
    o64, _ = oracles
    check_cond_pullback(pkg, o64, spec_of(o64, kw), alg, nsteps, B, path=2)


def test_layerwise_ys_bar_with_recomputed_activations(pkg, oracles):
    """The same sweep with the activations of a stage recomputed in the reverse pass instead of kept (layered_act_gib = 0)."""
    kw, alg, nsteps, B = LAYERED["swish / ELU chain"]
    o64, _ = oracles
    spec = spec_of(o64, kw)
    pkg.set_tuning(layered_act_gib=0)      # (restored by conftest's autouse fixture)
    check_cond_pullback(pkg, o64, spec, alg, nsteps, B, path=2)


# ---- 3. properties of the entries themselves, on both paths ----
BOTH = [(dict(nvars=8, ncond=8, hidden=[64, 64, 64], acts=1, reg_z=True, reg_j=True), 1),
        (dict(nvars=4, ncond=3, hidden=[32, 48], acts=[7, 4], reg_z=True, reg_j=True), 2)]


class Raw:
    """The C entries called directly on column-major device tensors."""

    def __init__(self, pkg, o64, kw, path, B, alg=1, nsteps=3, seed=11, ys=None):
        self.pkg, self.spec, self.B, self.alg, self.nsteps = pkg, spec_of(o64, kw), B, alg, nsteps
        spec = self.spec
        self.p, u0, eps, y, bar = inputs(o64, spec, B, seed)
        if ys is not None:
            y = ys
        self.ys = y
        self.icnf = make_icnf(pkg, spec, alg, nsteps)
        self.mode = mode_of(pkg, spec)
        assert pkg.vjp_path(self.icnf, self.mode, B, alg) == path
        self.h = self.icnf._handle(self.mode)
        self.ps = dev(self.p)
        self.icnf._bind_params(self.h, self.ps)
        col = lambda a: None if a is None else dev(np.ascontiguousarray(np.asarray(a).T))   # noqa: E731
        self.u0, self.eps, self.y, self.bar = col(u0), col(eps), col(y), col(bar)

    def call(self, entry, ys_bar=None, u0_bar="new", u1="new", y=None):
        """entry: "old" (cnf_integrate_fixed_vjp) or "cond"; returns (rc, grad, u0_bar, u1)."""
        lib, ptr = self.h.lib, self.pkg._lib.ptr
        grad = torch.empty(self.ps.numel(), device="cuda:0")
        u0_bar = torch.empty_like(self.u0) if isinstance(u0_bar, str) else u0_bar
        u1 = torch.empty_like(self.u0) if isinstance(u1, str) else u1
        y = self.y if y is None else y
        sp = self.pkg._lib.stream_ptr(torch.device("cuda:0"))
        head = (self.h.ptr, self.alg, self.nsteps, 0.0, 1.0, ptr(self.u0), ptr(self.eps), ptr(y), self.B, ptr(self.bar), ptr(grad), ptr(u0_bar))
        if entry == "old":
            rc = lib.cnf_integrate_fixed_vjp(*head, ptr(u1), sp)
        else:
            rc = lib.cnf_integrate_fixed_vjp_cond(*head, ptr(ys_bar), ptr(u1), sp)
        torch.cuda.synchronize()
        return rc, grad, u0_bar, u1


@pytest.mark.parametrize("kw,path", BOTH)
def test_null_is_the_old_entry_and_set_agrees_with_it(kw, path, pkg, oracles):
    o64, _ = oracles
    B = 37                                                  # no multiple of 16
    r = Raw(pkg, o64, kw, path, B)
    C_ = r.spec.ncond
    rc, g_old, ub_old, u1_old = r.call("old")
    assert rc == 0
    rc, g_null, ub_null, u1_null = r.call("cond", None)
    assert rc == 0
    assert torch.equal(g_null, g_old) and torch.equal(ub_null, ub_old) and torch.equal(u1_null, u1_old)     # bit for bit
    # ys_bar with a guard tail of sentinels behind its C B floats
    tail = 64
    buf = torch.full((B * C_ + tail,), 7.5, device="cuda:0")
    rc, g_set, ub_set, u1_set = r.call("cond", buf)
    assert rc == 0
    assert torch.all(buf[B * C_:] == 7.5)
    assert torch.isfinite(buf[:B * C_]).all() and not torch.any(buf[:B * C_] == 7.5)
    grad_close(g_set.cpu().numpy(), g_null.cpu().numpy(), "grad: ys_bar set vs NULL")
    grad_close(ub_set.cpu().numpy(), ub_null.cpu().numpy(), "u0_bar: ys_bar set vs NULL")
    assert float((u1_set - u1_null).abs().max()) < TOL_SOLVE
    # two identical calls are bitwise equal
    buf2 = torch.full((B * C_ + tail,), 7.5, device="cuda:0")
    rc, g_set2, ub_set2, u1_set2 = r.call("cond", buf2)
    assert rc == 0
    assert torch.equal(buf2, buf) and torch.equal(g_set2, g_set) and torch.equal(ub_set2, ub_set) and torch.equal(u1_set2, u1_set)


@pytest.mark.parametrize("kw,path", BOTH)
def test_unit_conditions_identity_with_the_weight_gradient(kw, path, pkg, oracles):
    """No oracle: with every column's ys = e_k, grad_{W_1}[:, ycol k] = sum_j (sum over stages of sbar_1[:, j]) and
    sum_j ys_bar[:, j] = W_1[:, ycols]^T of the same sum."""
    o64, _ = oracles
    spec = spec_of(o64, kw)
    B, k = 37, 1
    ys = np.zeros((spec.ncond, B), np.float32)
    ys[k] = 1.0
    r = Raw(pkg, o64, kw, path, B, ys=ys)
    ys_bar = torch.empty(B, spec.ncond, device="cuda:0")
    rc, g, _, _ = r.call("cond", ys_bar)
    assert rc == 0
    w_off = spec.param_offsets()[0]
    H, n_in = spec.widths[1], spec.widths[0]
    ycol = spec.D + (0 if spec.autonomous else 1)
    W1 = np.asarray(r.p, np.float64)[w_off[0]:w_off[0] + n_in * H].reshape(n_in, H).T          # H x n_in
    gW1 = g.cpu().numpy().astype(np.float64)[w_off[0]:w_off[0] + n_in * H].reshape(n_in, H).T
    want = W1[:, ycol:ycol + spec.ncond].T @ gW1[:, ycol + k]
    got = ys_bar.cpu().numpy().astype(np.float64).sum(0)
    grad_close(got, want, "sum_j ys_bar vs W_1[:, ycols]^T grad_W1[:, ycol k]")


@pytest.mark.parametrize("kw,path", BOTH)
def test_error_returns(kw, path, pkg, oracles):
    o64, _ = oracles
    INV = pkg._lib.ERR_INVALID
    B = 20
    r = Raw(pkg, o64, kw, path, B)
    good = torch.empty(B, r.spec.ncond, device="cuda:0")
    S = r.spec.D + 3
    # aliasing: ys, u0, u1_bar, u0_bar, u1
    assert r.call("cond", r.y)[0] == INV
    assert "alias" in r.h.lib.cnf_last_error().decode()
    assert r.call("cond", r.u0)[0] == INV
    assert r.call("cond", r.bar)[0] == INV
    shared = torch.empty(B, max(S, r.spec.ncond), device="cuda:0")
    assert r.call("cond", shared, u0_bar=shared)[0] == INV
    assert r.call("cond", shared, u1=shared)[0] == INV
    assert r.call("cond", good)[0] == 0
    # an unconditioned handle
    kw0 = {k: v for k, v in kw.items() if k != "ncond"}
    r0 = Raw(pkg, o64, kw0, path, B)
    assert r0.call("cond", None)[0] == 0
    assert r0.call("cond", torch.empty(B, 4, device="cuda:0"))[0] == INV
    assert "no conditions" in r0.h.lib.cnf_last_error().decode()


def test_zero_columns_zero_grad_and_touch_nothing_else(pkg, oracles):
    o64, _ = oracles
    kw, path = BOTH[0]
    r = Raw(pkg, o64, kw, path, 20)
    r.B = 0
    ys_bar = torch.full((20 * r.spec.ncond,), 7.5, device="cuda:0")
    u0_bar = torch.full_like(r.u0, 7.5)
    rc, g, ub, _ = r.call("cond", ys_bar, u0_bar=u0_bar)
    assert rc == 0 and torch.all(g == 0.0) and torch.all(ys_bar == 7.5) and torch.all(ub == 7.5)


# ---- 4. autograd on top: an encoder in front of the conditions ----
AUTOGRAD = [(dict(nvars=3, ncond=2, hidden=[32, 32], acts=1), 1), (dict(nvars=3, ncond=2, hidden=[32, 32], acts=7), 2)]


def encoder(spec, B, seed, R=5):
    rng = np.random.default_rng(seed)
    return (0.5 * rng.standard_normal((spec.ncond, R))).astype(np.float32), (0.1 * rng.standard_normal(spec.ncond)).astype(np.float32), \
        rng.standard_normal((R, B)).astype(np.float32)


def check_inference_grads(pkg, o64, spec, icnf, B, nsteps, alg, adaptive):
    p, xs, eps, _ = o64.synth_inputs(spec, B, 21, bias_scale=0.2)
    We, be, r = encoder(spec, B, 5)
    m = pkg.TrainMode(False)
    W, b, ps, x = dev(We).requires_grad_(), dev(be).requires_grad_(), dev(p).requires_grad_(), dev(xs).requires_grad_()
    ys = W @ dev(r) + b[:, None]
    with pytest.raises(NotImplementedError, match="cond_grad=True"):        # without the keyword the refusal stands
        pkg.inference(icnf, m, x, ys, ps, {}, eps=dev(eps), differentiable=True)
    lp = pkg.inference(icnf, m, x, ys, ps, {}, eps=dev(eps), differentiable=True, cond_grad=True)[0]
    grid = list(icnf.last_solve_stats["tgrid"]) if adaptive else None
    if adaptive:
        assert len(grid) >= 3 and grid[0] == 0.0 and grid[-1] == 1.0
    L = -lp.mean()
    L.backward()
    Wt, bt, pt, xt = cref.leaf(We), cref.leaf(be), cref.leaf(p), cref.leaf(xs)
    yt = Wt @ cref.leaf(r, False) + bt[:, None]
    u0 = torch.cat([xt, torch.zeros(3, B, dtype=torch.float64)], 0)
    u1 = cref.integrate(o64, spec, pt, u0, yt, 0.0, 1.0, None if adaptive else nsteps, alg, eps, tgrid=grid)
    D = spec.D
    Lr = -(-0.5 * D * np.log(2.0 * np.pi) - 0.5 * (u1[:D] * u1[:D]).sum(0) - u1[D]).mean()
    rW, rb, rp, rx = torch.autograd.grad(Lr, (Wt, bt, pt, xt))
    assert abs(float(L.detach()) - float(Lr.detach())) < TOL_SOLVE
    grad_close(W.grad.cpu().numpy(), rW.numpy(), "W_enc")
    grad_close(b.grad.cpu().numpy(), rb.numpy(), "b_enc")
    grad_close(ps.grad.cpu().numpy(), rp.numpy(), "ps")
    grad_close(x.grad.cpu().numpy(), rx.numpy(), "xs")


@pytest.mark.parametrize("kw,path", AUTOGRAD)
def test_autograd_through_an_encoder_fixed_step(kw, path, pkg, oracles):
    o64, _ = oracles
    spec = spec_of(o64, kw)
    B, nsteps, alg = 40, 4, 1
    icnf = make_icnf(pkg, spec, alg, nsteps)
    assert pkg.vjp_path(icnf, pkg.TrainMode(False), B, alg) == path
    check_inference_grads(pkg, o64, spec, icnf, B, nsteps, alg, adaptive=False)


@pytest.mark.parametrize("kw,path", AUTOGRAD)
def test_autograd_through_an_encoder_under_adaptive_tsit5(kw, path, pkg, oracles):
    """The backward runs on the grid the forward accepted (last_solve_stats["tgrid"]), as for ps."""
    o64, _ = oracles
    spec = spec_of(o64, kw)
    B = 32
    icnf = make_icnf(pkg, spec, 1, 4)
    icnf.sol_kwargs = dict(alg=pkg.Tsit5(), abstol=1e-5, reltol=1e-5)
    assert icnf.adaptive
    assert pkg.vjp_path(icnf, pkg.TrainMode(False), B, 1, True) == path
    check_inference_grads(pkg, o64, spec, icnf, B, None, 1, adaptive=True)


@pytest.mark.parametrize("kw,path", AUTOGRAD)
def test_autograd_through_generate(kw, path, pkg, oracles):
    o64, _ = oracles
    spec = spec_of(o64, kw)
    n, nsteps, alg = 36, 4, 1
    p, _, eps, _ = o64.synth_inputs(spec, n, 9, bias_scale=0.2)
    We, be, r = encoder(spec, n, 6)
    z0 = np.random.default_rng(2).standard_normal((spec.D, n)).astype(np.float32)
    icnf = make_icnf(pkg, spec, alg, nsteps)
    m = pkg.TrainMode(False)
    assert pkg.vjp_path(icnf, m, n, alg) == path
    W, b, ps, z = dev(We).requires_grad_(), dev(be).requires_grad_(), dev(p).requires_grad_(), dev(z0).requires_grad_()
    ys = W @ dev(r) + b[:, None]
    x = pkg.generate(icnf, m, ys, ps, {}, n, z0=z, eps=dev(eps), differentiable=True, cond_grad=True)
    plain = pkg.generate(icnf, m, ys.detach(), dev(p), {}, n, z0=dev(z0), eps=dev(eps))
    assert x.shape == (spec.nvars, n) and float((x.detach() - plain).abs().max()) < TOL_SOLVE
    L = (x * x).sum(0).mean()
    L.backward()
    Wt, bt, pt, zt = cref.leaf(We), cref.leaf(be), cref.leaf(p), cref.leaf(z0)
    yt = Wt @ cref.leaf(r, False) + bt[:, None]
    u0 = torch.cat([zt, torch.zeros(3, n, dtype=torch.float64)], 0)
    xr = cref.integrate(o64, spec, pt, u0, yt, 1.0, 0.0, nsteps, alg, eps)[:spec.nvars]
    Lr = (xr * xr).sum(0).mean()
    rW, rb, rp, rz = torch.autograd.grad(Lr, (Wt, bt, pt, zt))
    assert abs(float(L.detach()) - float(Lr.detach())) < TOL_SOLVE
    grad_close(W.grad.cpu().numpy(), rW.numpy(), "generate: W_enc")
    grad_close(b.grad.cpu().numpy(), rb.numpy(), "generate: b_enc")
    grad_close(ps.grad.cpu().numpy(), rp.numpy(), "generate: ps")
    grad_close(z.grad.cpu().numpy(), rz.numpy(), "generate: z0")
