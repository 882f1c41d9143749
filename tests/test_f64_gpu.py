"""GPU: Float64 flows - the double-precision entries of the C ABI (cnf_set_params_f64, cnf_aug_f_f64, cnf_integrate_fixed_f64,
cnf_inference_fixed_f64: one kernel, csrc/cnf_f64.hip, every product on v_mfma_f64_16x16x4_f64) and ICNF(data_type=torch.float64)
on top of them, against the fp64 oracle (oracle/cnf_oracle64.py).

Tolerance: |got - ref| <= 1e-9 max(1, max|ref|) for states, logp and regs.  Both sides are double and differ by summation order
and libm only (contractions <= 640 long, <= 240 stage evaluations: expected <~ 1e-12), while one f32 product, tableau coefficient
or stage time anywhere in the chain shows at >= 1e-7 - the bound is met by computing in double throughout and not otherwise.
The inputs carry low-order bits a Float32 cannot hold (`jitter`), so a load through float would show as well.  Every case prints
its measured error.  The oracle knows identity / tanh / softplus; the fixture below adds the other four activations to it in
plain torch float64 (the formulas of include/cnf.h), differentiated by torch.autograd like the rest of the chain."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL64 = 1e-9
TOL_SOLVE = 1e-4      # the project's bound between two implementations of a Float32 solve (tests/test_activations_gpu.py)
NAMES = {0: "identity", 1: "tanh", 2: "softplus", 4: "sigmoid", 5: "swish", 6: "elu", 7: "gelu"}
VJP, JVP, EXACT = 0, 1, 2
RK4, TSIT5 = 0, 1


def _new_act(a, kind):
    if kind == 4:
        return torch.sigmoid(a)
    if kind == 5:
        return a * torch.sigmoid(a)
    if kind == 6:
        return torch.where(a >= 0, a, torch.expm1(a))
    if kind == 7:
        return torch.nn.functional.gelu(a, approximate="tanh")
    return None


@pytest.fixture
def o64(oracles, monkeypatch):
    mod, _ = oracles
    base = mod._act

    def act(a, kind):
        h = _new_act(a, kind)
        return base(a, kind) if h is None else h

    monkeypatch.setattr(mod, "_act", act)
    return mod


def spec_of(o64, nvars, hidden, acts, **kw):
    s = o64.make_spec(nvars, hidden, **kw)
    if not isinstance(acts, int):
        s.acts = list(acts) + [0]
    else:
        s.acts = [acts] * len(hidden) + [0]
    s.check()
    return s


# name -> (spec arguments, alg, nsteps, B): the cases of the issue, the smallest shapes at which the kernel can still go wrong
CASES = {
    # M padding 10 -> 16 and 37 -> 48, K padding 10 -> 12 and 37 -> 40, a ragged second tile
    "1 padded widths": (dict(nvars=2, hidden=[10, 37], acts=[1, 2]), TSIT5, 3, 17),
    # the default net at nvariables = 1 (4-16-16-3 softplus, naug = 2) with all three regularisers
    "2 default net": (dict(nvars=1, hidden=[16, 16], acts=2, naug=2, reg_z=True, reg_j=True, reg_aug=True), RK4, 4, 50),
    "3 cfg2 shape": (dict(nvars=8, hidden=[64, 64, 64], acts=1), TSIT5, 5, 100),
    "3 cfg2 shape, one column": (dict(nvars=8, hidden=[64, 64, 64], acts=1), TSIT5, 5, 1),
    "4 conditioned, autonomous, two probes": (dict(nvars=3, hidden=[24, 24, 24], acts=1, ncond=2, autonomous=True, nprobes=2,
                                                   reg_z=True, reg_j=True), RK4, 3, 19),
    "5 exact trace": (dict(nvars=4, hidden=[32, 32], acts=1, mode=EXACT), TSIT5, 3, 18),
    # several M tiles; one wave per workgroup (the fewest-waves end of the LDS budget)
    "6 wide": (dict(nvars=5, hidden=[200, 72], acts=1), RK4, 2, 33),
    "7 sigmoid, swish": (dict(nvars=2, hidden=[10, 37], acts=[4, 5]), TSIT5, 3, 17),
    "7 swish, elu": (dict(nvars=2, hidden=[10, 37], acts=[5, 6]), TSIT5, 3, 17),
    "7 elu, gelu": (dict(nvars=2, hidden=[10, 37], acts=[6, 7]), TSIT5, 3, 17),
    "7 gelu, sigmoid": (dict(nvars=2, hidden=[10, 37], acts=[7, 4]), TSIT5, 3, 17),
}


def inputs(o64, spec, B, seed=17):
    """(p, xs, eps, ys) in float64 with low-order bits beyond Float32."""
    p, xs, eps, ys = o64.synth_inputs(spec, B, seed=seed, bias_scale=0.2)
    rng = np.random.default_rng(seed + 1000)
    jitter = lambda a: None if a is None else a.astype(np.float64) * (1.0 + 1e-9 * rng.standard_normal(a.shape))
    return jitter(p), jitter(xs), jitter(eps), jitter(ys)


_cache = {}


def case(o64, name):
    """The case's spec, inputs and oracle solve, computed once and shared (nothing writes to them)."""
    if name not in _cache:
        kw, alg, nsteps, B = CASES[name]
        kw = dict(kw)
        spec = spec_of(o64, kw.pop("nvars"), kw.pop("hidden"), kw.pop("acts"), **kw)
        p, xs, eps, ys = inputs(o64, spec, B)
        e = None if spec.mode == EXACT else eps
        logp, regs, u1 = o64.inference_fixed(spec, p, xs, 0.0, 1.0, nsteps, alg, e, ys)
        for a in (p, xs, eps, logp, u1) + tuple(regs) + (() if ys is None else (ys,)):
            a.setflags(write=False)
        _cache[name] = (spec, alg, nsteps, B, p, xs, e, ys, logp, regs, u1)
    return _cache[name]


def dev(a):
    """(rows, B) float64 array -> the column-major device array the ABI takes ((B, rows) contiguous)."""
    return None if a is None else torch.tensor(np.ascontiguousarray(np.asarray(a, dtype=np.float64).T), device="cuda:0")


def ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


class Flow:
    """One cnf_handle with its Float64 parameter binding, driven through ctypes."""

    def __init__(self, pkg, spec, p=None):
        self.L, self.lib, self.spec = pkg._lib, pkg._lib.load(), spec
        cfg = self.L.CnfConfig()
        cfg.nvars, cfg.naug, cfg.ncond, cfg.autonomous, cfg.n_layers = spec.nvars, spec.naug, spec.ncond, int(spec.autonomous), len(spec.acts)
        for i, w in enumerate(spec.widths):
            cfg.widths[i] = w
        for i, a in enumerate(spec.acts):
            cfg.acts[i] = a
        cfg.mode, cfg.nprobes = spec.mode, spec.nprobes
        cfg.reg_z, cfg.reg_j, cfg.reg_aug = int(spec.reg_z), int(spec.reg_j), int(spec.reg_aug)
        self.h = C.c_void_p()
        self.L.check(self.lib.cnf_create(C.byref(self.h), C.byref(cfg)))
        if p is not None:
            self.L.check(self.set_params(p))

    def set_params(self, p, on_device=True):
        w_off, b_off, n = self.spec.param_offsets()
        wo, bo = (C.c_size_t * len(w_off))(*w_off), (C.c_size_t * len(b_off))(*b_off)
        if on_device:
            self.p = torch.tensor(p, device="cuda:0", dtype=torch.float64)
            return self.lib.cnf_set_params_f64(self.h, ptr(self.p), n, wo, bo, 1, None)
        host = np.ascontiguousarray(p, dtype=np.float64)
        return self.lib.cnf_set_params_f64(self.h, C.c_void_p(host.ctypes.data), n, wo, bo, 0, None)

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.cnf_destroy(self.h)

    def aug_f(self, u, t, eps, ys):
        um, e, y = dev(u), dev(eps), dev(ys)
        du = torch.empty_like(um)
        self.L.check(self.lib.cnf_aug_f_f64(self.h, ptr(du), ptr(um), t, ptr(e), ptr(y), um.shape[0], None))
        return du.cpu().numpy().T

    def integrate(self, alg, nsteps, t0, t1, u0, eps, ys, alias=False):
        um, e, y = dev(u0), dev(eps), dev(ys)
        u1 = um if alias else torch.empty_like(um)
        self.L.check(self.lib.cnf_integrate_fixed_f64(self.h, alg, nsteps, t0, t1, ptr(um), ptr(e), ptr(y), um.shape[0], ptr(u1), None))
        return u1.cpu().numpy().T

    def inference(self, alg, nsteps, xs, eps, ys, t0=0.0, t1=1.0):
        x, e, y = dev(xs), dev(eps), dev(ys)
        B = x.shape[0]
        logp = torch.empty(B, device="cuda:0", dtype=torch.float64)
        regs = torch.empty(3, B, device="cuda:0", dtype=torch.float64)
        uf = torch.empty(B, self.spec.S, device="cuda:0", dtype=torch.float64)
        self.L.check(self.lib.cnf_inference_fixed_f64(self.h, alg, nsteps, t0, t1, ptr(x), ptr(e), ptr(y), B, ptr(logp), ptr(regs), ptr(uf), None))
        return logp.cpu().numpy(), regs.cpu().numpy(), uf.cpu().numpy().T


def close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = max(1.0, float(np.abs(want).max()))
    err = float(np.abs(got - want).max())
    print(f"{what}: max|got - ref| = {err:.3e} (max|ref| = {np.abs(want).max():.3e}; bound {TOL64 * scale:.1e})")
    assert np.isfinite(got).all(), what
    assert err <= TOL64 * scale, (what, err)


# ---- cases 1 - 7: the whole solve, inference form (logp, regs with Adot, final state) ----
@pytest.mark.parametrize("name", sorted(CASES))
def test_inference_matches_the_oracle(name, pkg, o64):
    spec, alg, nsteps, B, p, xs, eps, ys, logp, regs, u1 = case(o64, name)
    f = Flow(pkg, spec, p)
    assert f.lib.cnf_f64_supported(f.h) == 1
    got_logp, got_regs, got_u = f.inference(alg, nsteps, xs, eps, ys)
    close(got_u, u1, f"{name}: state")
    close(got_logp, logp, f"{name}: logp")
    for i, what in enumerate(("Edot", "ndot", "Adot")):
        close(got_regs[i], regs[i], f"{name}: {what}")
    if spec.reg_aug:
        assert np.abs(regs[2]).min() > 0.0       # Adot is live in the case that has it
    # NULL regs / u_final: logp alone, the same bits
    x, e, y = dev(xs), dev(eps), dev(ys)
    lp = torch.empty(B, device="cuda:0", dtype=torch.float64)
    f.L.check(f.lib.cnf_inference_fixed_f64(f.h, alg, nsteps, 0.0, 1.0, ptr(x), ptr(e), ptr(y), B, ptr(lp), None, None, None))
    assert np.array_equal(lp.cpu().numpy(), got_logp)


def test_host_parameters_give_the_same_bits_as_device_parameters(pkg, o64):
    spec, alg, nsteps, B, p, xs, eps, ys, logp, regs, u1 = case(o64, "1 padded widths")
    a, b = Flow(pkg, spec, p), Flow(pkg, spec)
    assert b.set_params(p, on_device=False) == 0
    assert np.array_equal(a.inference(alg, nsteps, xs, eps, ys)[2], b.inference(alg, nsteps, xs, eps, ys)[2])


# ---- case 7, second half: pre-activations up to |a| = 50 (the stable forms) ----
@pytest.mark.parametrize("name", [n for n in sorted(CASES) if n.startswith("7")])
def test_large_preactivations_stay_finite_and_exact(name, pkg, o64):
    spec, alg, nsteps, B, p, xs, eps, ys, *_ = case(o64, name)
    (W, b), = o64.unpack_params(spec, p)[:1]
    rng = np.random.default_rng(3)
    z = rng.standard_normal((spec.D, B))
    t = 0.3
    a1 = W.numpy() @ np.vstack([z, np.full((1, B), t)]) + b.numpy()[:, None]
    z *= 50.0 / np.abs(a1).max()                               # layer one's pre-activations now reach about +-50
    a1 = W.numpy() @ np.vstack([z, np.full((1, B), t)]) + b.numpy()[:, None]
    assert 40.0 < np.abs(a1).max() < 60.0 and a1.min() < -30.0 and a1.max() > 30.0
    u = np.vstack([z, rng.standard_normal((3, B))])
    ref = o64.aug_f(spec, p, u, t, eps, ys)
    close(Flow(pkg, spec, p).aug_f(u, t, eps, ys), ref, f"{name}: aug_f at |a| <= {np.abs(a1).max():.0f}")


# ---- case 8: one dynamics call ----
@pytest.mark.parametrize("name", ["1 padded widths", "4 conditioned, autonomous, two probes", "5 exact trace"])
def test_aug_f_matches_the_oracle(name, pkg, o64):
    spec, alg, nsteps, B, p, xs, eps, ys, *_ = case(o64, name)
    rng = np.random.default_rng(5)
    u = np.vstack([xs, rng.standard_normal((spec.naug + 3, B))])
    ref = o64.aug_f(spec, p, u, 0.3, eps, ys)
    close(Flow(pkg, spec, p).aug_f(u, 0.3, eps, ys), ref, f"{name}: aug_f")


# ---- case 9: backwards, and u1 aliasing u0 ----
def test_backwards_solve_and_aliased_output(pkg, o64):
    spec, alg, nsteps, B, p, xs, eps, ys, logp, regs, u1 = case(o64, "1 padded widths")
    ref = o64.integrate_fixed(spec, p, u1, 1.0, 0.0, nsteps, alg, eps, ys)
    f = Flow(pkg, spec, p)
    back = f.integrate(alg, nsteps, 1.0, 0.0, u1, eps, ys)
    close(back, ref, "backwards solve")
    assert np.array_equal(f.integrate(alg, nsteps, 1.0, 0.0, u1, eps, ys, alias=True), back)      # bit for bit
    fwd = f.integrate(alg, nsteps, 0.0, 1.0, np.vstack([xs, np.zeros((spec.naug + 3, B))]), eps, ys)
    close(fwd, u1, "integrate form of the forward solve")
    assert np.array_equal(f.integrate(alg, nsteps, 0.0, 1.0, np.vstack([xs, np.zeros((spec.naug + 3, B))]), eps, ys, alias=True), fwd)


# ---- case 10: a column's result does not depend on the other columns of the call ----
def test_columns_are_independent_bit_for_bit(pkg, o64):
    spec, alg, nsteps, B, p, xs, eps, ys, *_ = case(o64, "2 default net")
    f = Flow(pkg, spec, p)
    full = f.inference(alg, nsteps, xs, eps, ys)
    part = f.inference(alg, nsteps, xs[:, :17], eps[:, :17], None)
    assert np.array_equal(full[0][:17], part[0])
    assert np.array_equal(full[1][:, :17], part[1])
    assert np.array_equal(full[2][:, :17], part[2])


# ---- case 11: the shipped Float32 path on the same inputs, an independent implementation ----
@pytest.mark.parametrize("name", ["2 default net", "3 cfg2 shape", "4 conditioned, autonomous, two probes"])
def test_agrees_with_the_float32_path(name, pkg, o64):
    spec, alg, nsteps, B, *_ = case(o64, name)
    p, xs, eps, ys = o64.synth_inputs(spec, B, seed=23, bias_scale=0.2)            # Float32 values: the same numbers on both sides
    d64 = lambda a: None if a is None else a.astype(np.float64)
    logp, regs, u = Flow(pkg, spec, d64(p)).inference(alg, nsteps, d64(xs), d64(eps), d64(ys))
    icnf = make_icnf(pkg, spec, alg, nsteps, torch.float32)
    t32 = lambda a: torch.tensor(a, device="cuda:0")
    args = (t32(xs),) + ((t32(ys),) if spec.ncond else ()) + (t32(p), {})
    l32, (E, n, A), u32 = pkg.inference(icnf, mode_of(pkg, spec), *args, eps=t32(eps), return_state=True)
    for got, want, what in ((l32, logp, "logp"), (E, regs[0], "Edot"), (n, regs[1], "ndot"), (A, regs[2], "Adot"), (u32, u, "state")):
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
        print(f"{name}: Float32 path vs Float64 path, {what}: {err:.3e}")
        assert err < TOL_SOLVE, (what, err)


# ---- case 12: the Python surface ----
def make_icnf(pkg, spec, alg, nsteps, dtype, **sol):
    layers = [pkg.Dense(spec.widths[i], spec.widths[i + 1], NAMES[spec.acts[i]]) for i in range(len(spec.acts))]
    sol_kwargs = dict(alg=pkg.Tsit5() if alg == TSIT5 else pkg.RK4(), adaptive=False)
    sol_kwargs.update(sol or dict(nsteps=nsteps))
    return pkg.ICNF(data_type=dtype, nvariables=spec.nvars, naugments=spec.naug, nconditions=spec.ncond, autonomous=spec.autonomous,
                    nn=pkg.Chain(*layers), steer_rate=0.0, lambda1=0.01 if spec.reg_z else 0.0, lambda2=0.02 if spec.reg_j else 0.0,
                    lambda3=0.03 if spec.reg_aug else 0.0, nprobes=spec.nprobes, device="cuda:0", sol_kwargs=sol_kwargs)


def mode_of(pkg, spec):
    return pkg.TestMode() if spec.mode == EXACT else pkg.TrainMode(bool(spec.reg_z or spec.reg_j or spec.reg_aug))


def t64(a):
    return None if a is None else torch.tensor(np.asarray(a), device="cuda:0", dtype=torch.float64)


@pytest.mark.parametrize("name", ["2 default net", "4 conditioned, autonomous, two probes"])
def test_python_surface(name, pkg, o64):
    spec, alg, nsteps, B, p, xs, eps, ys, logp, regs, u1 = case(o64, name)
    icnf = make_icnf(pkg, spec, alg, nsteps, torch.float64)
    mode = mode_of(pkg, spec)
    cond = (t64(ys),) if spec.ncond else ()
    ps = t64(p)
    # inference
    got_logp, got_regs, got_u = pkg.inference(icnf, mode, t64(xs), *cond, ps, {}, eps=t64(eps), return_state=True)
    assert got_logp.dtype == torch.float64 and got_u.dtype == torch.float64 and all(r.dtype == torch.float64 for r in got_regs)
    close(got_logp.cpu().numpy(), logp, f"{name}: inference logp")
    close(got_u.cpu().numpy(), u1, f"{name}: inference state")
    for i in range(3):
        close(got_regs[i].cpu().numpy(), regs[i], f"{name}: inference regs[{i}]")
    # loss: the mean in torch float64
    lam = (icnf.lambda1, icnf.lambda2, icnf.lambda3)
    want = float(np.mean(-logp + lam[0] * regs[0] + lam[1] * regs[1] + lam[2] * regs[2]))
    got = pkg.loss(icnf, mode, t64(xs), *cond, ps, {}, eps=t64(eps))
    assert got.dtype == torch.float64 and got.dim() == 0
    close(got.item(), want, f"{name}: loss")
    # augmented_f
    u = np.vstack([xs, np.random.default_rng(5).standard_normal((spec.naug + 3, B))])
    du = pkg.augmented_f(icnf, mode, t64(u), ps, 0.3, t64(eps), *([t64(ys)] if spec.ncond else []))
    assert du.dtype == torch.float64
    close(du.cpu().numpy(), o64.aug_f(spec, p, u, 0.3, eps, ys), f"{name}: augmented_f")
    # generate runs the reversed span: against the oracle's backwards solve from the same base points ...
    z0 = u1[:spec.D]
    gen = pkg.generate(icnf, mode, *cond, ps, {}, B, z0=t64(z0), eps=t64(eps))
    assert gen.dtype == torch.float64 and tuple(gen.shape) == (spec.nvars, B)
    back = o64.integrate_fixed(spec, p, np.vstack([z0, np.zeros((3, B))]), 1.0, 0.0, nsteps, alg, eps, ys)
    close(gen.cpu().numpy(), back[:spec.nvars], f"{name}: generate")
    # ... and, on steps fine enough that the truncation error of the round trip is far below the bound (Tsit5 is fifth order: at
    # 100 steps h^5 = 1e-10 times an error constant of order 1e-3 for these small nets), generate inverts inference
    fine = make_icnf(pkg, spec, TSIT5, 100, torch.float64)
    _, _, uf = pkg.inference(fine, mode, t64(xs), *cond, ps, {}, eps=t64(eps), return_state=True)
    inv = pkg.generate(fine, mode, *cond, ps, {}, B, z0=uf[:spec.D].contiguous(), eps=t64(eps))
    close(inv.cpu().numpy(), xs, f"{name}: generate(inference(xs))")
    # dt = 0.3 on (0, 1): three full steps and a tail step
    tail = make_icnf(pkg, spec, alg, 0, torch.float64, dt=0.3)
    lt, rt, ut = pkg.inference(tail, mode, t64(xs), *cond, ps, {}, eps=t64(eps), return_state=True)
    wl, wr, wu = o64.inference_fixed(spec, p, xs, 0.0, 1.0, 0, alg, eps, ys, dt=0.3)
    close(ut.cpu().numpy(), wu, f"{name}: dt = 0.3, state")
    close(lt.cpu().numpy(), wl, f"{name}: dt = 0.3, logp")
    for i in range(3):
        close(rt[i].cpu().numpy(), wr[i], f"{name}: dt = 0.3, regs[{i}]")
    u0 = np.vstack([xs, np.zeros((spec.naug + 3, B))])
    close(ut.cpu().numpy(), o64.integrate_fixed_dt(spec, p, u0, 0.0, 1.0, 0.3, alg, eps, ys), f"{name}: dt = 0.3 against integrate_fixed_dt")


@pytest.mark.parametrize("name", ["2 default net", "4 conditioned, autonomous, two probes"])
def test_dist_logpdf_and_rand(name, pkg, o64):
    """ICNFDist / CondICNFDist in TestMode: the exact trace."""
    spec, alg, nsteps, B, p, xs, eps, ys, *_ = case(o64, name)
    icnf = make_icnf(pkg, spec, alg, nsteps, torch.float64)
    ex = o64.Spec(nvars=spec.nvars, naug=spec.naug, ncond=spec.ncond, autonomous=spec.autonomous, widths=spec.widths, acts=spec.acts, mode=EXACT)
    want, _, _ = o64.inference_fixed(ex, p, xs, 0.0, 1.0, nsteps, alg, None, ys)
    if spec.ncond:
        d = pkg.CondICNFDist(icnf, pkg.TestMode(), t64(ys), t64(p), {})
    else:
        d = pkg.ICNFDist(icnf, pkg.TestMode(), t64(p), {})
    got = d.logpdf(t64(xs))
    assert got.dtype == torch.float64
    close(got.cpu().numpy(), want, f"{name}: logpdf")
    one = d.logpdf(t64(xs[:, 0]))
    assert one.dim() == 0 and one.item() == got[0].item()
    r = d.rand(5)
    assert r.dtype == torch.float64 and tuple(r.shape) == (spec.nvars, 5) and torch.isfinite(r).all()


# ---- case 13: refusals ----
def test_refusals(pkg, o64):
    lib, L = pkg._lib.load(), pkg._lib
    # JVP mode
    jvp = spec_of(o64, 2, [10, 37], [1, 2], mode=JVP)
    f = Flow(pkg, jvp)
    assert lib.cnf_f64_supported(f.h) == 0 and "CNF_MODE_HUTCH_JVP" in lib.cnf_last_error().decode()
    p = inputs(o64, jvp, 4)[0]
    assert f.set_params(p) == L.ERR_UNSUPPORTED
    icnf = pkg.ICNF(data_type=torch.float64, nvariables=2, naugments=0, compute_mode=pkg.HIPJacVecMatrixMode(), device="cuda:0",
                    nn=pkg.Chain(pkg.Dense(3, 10, pkg.tanh), pkg.Dense(10, 2)), sol_kwargs=dict(alg=pkg.RK4(), adaptive=False, nsteps=2))
    ps = torch.zeros(52, device="cuda:0", dtype=torch.float64)
    with pytest.raises(L.CnfError, match="CNF_MODE_HUTCH_JVP"):
        pkg.inference(icnf, pkg.TrainMode(), torch.zeros(2, 4, device="cuda:0", dtype=torch.float64), ps, {})
    # a flow past the LDS limit: 128 bytes x (4 + (640 + 640 + 16) + 2 x 640 + 7 x 5 + 2) = 335 KB for one wave
    wide = spec_of(o64, 2, [640, 640], 1)
    w = Flow(pkg, wide)
    assert lib.cnf_f64_supported(w.h) == 0
    msg = lib.cnf_last_error().decode()
    assert "2617 LDS rows" in msg and "163840" in msg, msg
    assert w.set_params(np.zeros(wide.param_offsets()[2])) == L.ERR_UNSUPPORTED
    # the widest two-layer net of this kind that fits is supported: the limit is the formula, not a table
    assert lib.cnf_f64_supported(Flow(pkg, spec_of(o64, 2, [304, 304], 1)).h) == 1       # 4 + 624 + 608 + 35 + 2 = 1273 <= 1280
    assert lib.cnf_f64_supported(Flow(pkg, spec_of(o64, 2, [320, 304], 1)).h) == 0       # 4 + 640 + 640 + 35 + 2 = 1321
    # an f64 call before cnf_set_params_f64 - also when the Float32 binding exists
    spec, alg, nsteps, B, p, xs, eps, ys, *_ = case(o64, "1 padded widths")
    g = Flow(pkg, spec)
    w_off, b_off, n = spec.param_offsets()
    p32 = torch.tensor(p, device="cuda:0", dtype=torch.float32)
    L.check(lib.cnf_set_params(g.h, ptr(p32), n, (C.c_size_t * 3)(*w_off), (C.c_size_t * 3)(*b_off), 1, None))
    x, e = dev(xs), dev(eps)
    lp = torch.empty(B, device="cuda:0", dtype=torch.float64)
    assert lib.cnf_inference_fixed_f64(g.h, alg, nsteps, 0.0, 1.0, ptr(x), ptr(e), None, B, ptr(lp), None, None, None) == L.ERR_NO_PARAMS
    assert "cnf_set_params_f64" in lib.cnf_last_error().decode()
    u = torch.zeros(B, spec.S, device="cuda:0", dtype=torch.float64)
    assert lib.cnf_aug_f_f64(g.h, ptr(torch.empty_like(u)), ptr(u), 0.0, ptr(e), None, B, None) == L.ERR_NO_PARAMS
    assert lib.cnf_integrate_fixed_f64(g.h, alg, nsteps, 0.0, 1.0, ptr(u), ptr(e), None, B, ptr(u), None) == L.ERR_NO_PARAMS
    # ... and the Float64 binding does not stand in for the Float32 one
    h2 = Flow(pkg, spec, p)
    l32 = torch.empty(B, device="cuda:0", dtype=torch.float32)
    assert lib.cnf_inference_fixed(h2.h, alg, nsteps, 0.0, 1.0, ptr(x), ptr(e), None, B, ptr(l32), None, None, None) == L.ERR_NO_PARAMS
    # bad solver arguments
    assert lib.cnf_integrate_fixed_f64(h2.h, alg, 0, 0.0, 1.0, ptr(u), ptr(e), None, B, ptr(u), None) == L.ERR_INVALID
    assert lib.cnf_integrate_fixed_f64(h2.h, 2, 3, 0.0, 1.0, ptr(u), ptr(e), None, B, ptr(u), None) == L.ERR_INVALID
    assert lib.cnf_integrate_fixed_f64(h2.h, alg, 3, 0.0, 1.0, ptr(u), None, None, B, ptr(u), None) == L.ERR_INVALID      # no probes
    # dtype mismatches: a TypeError either way, nothing cast silently
    i64 = make_icnf(pkg, spec, alg, nsteps, torch.float64)
    i32 = make_icnf(pkg, spec, alg, nsteps, torch.float32)
    with pytest.raises(TypeError):
        pkg.inference(i64, pkg.TrainMode(), torch.tensor(xs, device="cuda:0", dtype=torch.float32), t64(p), {})
    with pytest.raises(TypeError):
        pkg.inference(i64, pkg.TrainMode(), t64(xs), p32, {})
    with pytest.raises(TypeError):
        pkg.inference(i32, pkg.TrainMode(), torch.tensor(xs, device="cuda:0", dtype=torch.float32), t64(p), {})


# ---- the edge of the LDS budget: the largest regions are launched, and the fit is asked per call ----
def test_the_largest_supported_region_runs(pkg, o64):
    """hidden [304, 304]: 1273 of 1280 rows under Tsit5 - 162 944 bytes of dynamic LDS, one wave per workgroup."""
    spec = spec_of(o64, 2, [304, 304], 1)
    p, xs, eps, ys = inputs(o64, spec, 17)
    f = Flow(pkg, spec, p)
    assert f.lib.cnf_f64_supported(f.h) == 1
    logp, regs, u1 = o64.inference_fixed(spec, p, xs, 0.0, 1.0, 1, TSIT5, eps, ys)
    got_logp, got_regs, got_u = f.inference(TSIT5, 1, xs, eps, ys)
    close(got_u, u1, "largest region: state")
    close(got_logp, logp, "largest region: logp")


def test_a_flow_that_fits_rk4_but_not_tsit5_is_refused_per_call(pkg, o64):
    """Five probes on hidden [304, 304]: 1281 rows with six stage derivatives (Tsit5), 1271 with four (RK4), 1256 with one
    (a dynamics call).  cnf_f64_supported answers for every solver (0); the entries ask for their own stage count."""
    lib, L = pkg._lib.load(), pkg._lib
    spec = spec_of(o64, 2, [304, 304], 1, nprobes=5)
    p, xs, eps, ys = inputs(o64, spec, 17)
    f = Flow(pkg, spec)
    assert lib.cnf_f64_supported(f.h) == 0 and "1281 LDS rows" in lib.cnf_last_error().decode()
    assert f.set_params(p) == 0
    u = np.vstack([xs, np.zeros((3, 17))])
    close(f.aug_f(u, 0.3, eps, ys), o64.aug_f(spec, p, u, 0.3, eps, ys), "RK4-only flow: aug_f")
    logp, regs, u1 = o64.inference_fixed(spec, p, xs, 0.0, 1.0, 1, RK4, eps, ys)
    got_logp, got_regs, got_u = f.inference(RK4, 1, xs, eps, ys)
    close(got_u, u1, "RK4-only flow: state")
    close(got_logp, logp, "RK4-only flow: logp")
    x, e = dev(xs), dev(eps)
    lp = torch.empty(17, device="cuda:0", dtype=torch.float64)
    assert lib.cnf_inference_fixed_f64(f.h, TSIT5, 1, 0.0, 1.0, ptr(x), ptr(e), None, 17, ptr(lp), None, None, None) == L.ERR_UNSUPPORTED
    assert "1281 LDS rows" in lib.cnf_last_error().decode() and "ns = 6" in lib.cnf_last_error().decode()


def test_float64_example_runs_end_to_end():
    """examples/float64_logpdf.py as its own process: fit in Float32, evaluate in Float64."""
    import json, os, subprocess, sys
    from conftest import ROOT
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "float64_logpdf.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(res["logpdf_float64"]) == 2 and all(np.isfinite(v) for v in res["logpdf_float64"])
    assert max(abs(v) for v in res["float32_minus_float64"]) < TOL_SOLVE
    assert res["generate_of_inference_minus_x"] < TOL64
    assert abs(res["log_likelihood_ratio_float64"] - (res["logpdf_float64"][0] - res["logpdf_float64"][1])) < 1e-12
