"""Sigmoid, swish, ELU and GELU hidden layers on the GPU (include/cnf.h CNF_ACT_SIGMOID .. CNF_ACT_GELU), against the fp64
oracle.  The oracle dispatches activations through cnf_oracle64._act; the fixture below extends it with ids 4-7 for the length of
a test.  These nets run layer-wise (csrc/cnf_layered.hip) or thread-per-sample: every fused plan finder refuses them, which the
shape-band cases assert, and a wrong route would show as a mismatch against the oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAMES = {0: "identity", 1: "tanh", 2: "softplus", 4: "sigmoid", 5: "swish", 6: "elu", 7: "gelu"}
NEW = (4, 5, 6, 7)
TOL_CALL = 2e-5
TOL_SOLVE = 1e-4
RECOMPUTE = {"CNF_LAYERED_ACT_GIB": "0", "CNF_LAYERED_NO_KCKPT": "1"}


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
    """The fp64 oracle with ids 4-7; `o64.zero_dd = True` makes every activation's act'' zero (act' then enters the graph as a
    constant), the reference of a gradient that drops the act'' term."""
    mod, _ = oracles
    base = mod._act

    def act(a, kind):
        h = _new_act(a, kind)
        if h is None:
            h = base(a, kind)
        if getattr(mod, "zero_dd", False) and kind != 0:
            x = a.detach().requires_grad_(True)
            with torch.enable_grad():
                (d,) = torch.autograd.grad(act_plain(x, kind).sum(), x)
            return h.detach() + (a - a.detach()) * d
        return h

    def act_plain(a, kind):
        h = _new_act(a, kind)
        return base(a, kind) if h is None else h

    monkeypatch.setattr(mod, "_act", act)
    monkeypatch.setattr(mod, "zero_dd", False, raising=False)
    return mod


def setsw(pkg, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    pkg.reload_tuning()


def spec_of(o64, nvars, hidden, acts, **kw):
    """make_spec with one activation per hidden layer (or one for all) and an identity output layer, or `acts` for every layer."""
    if isinstance(acts, int):
        acts = [acts] * len(hidden)
    s = o64.make_spec(nvars, hidden, **kw)
    s.acts = list(acts) + [0] * (len(hidden) + 1 - len(acts))
    s.check()
    return s


def make_icnf(pkg, spec, alg, nsteps, path=0, lambdas=(0.01, 0.01, 0.01), tspan=(0.0, 1.0)):
    layers = [pkg.Dense(spec.widths[i], spec.widths[i + 1], NAMES[spec.acts[i]]) for i in range(len(spec.acts))]
    cm = (pkg.HIPJacVecMatrixMode if spec.mode == 1 else pkg.HIPVecJacMatrixMode)(kernel_path=path)
    return pkg.ICNF(nvariables=spec.nvars, naugments=spec.naug, nconditions=spec.ncond, autonomous=spec.autonomous,
                    nn=pkg.Chain(*layers), compute_mode=cm, steer_rate=0.0, tspan=tspan,
                    lambda1=lambdas[0] if spec.reg_z else 0.0, lambda2=lambdas[1] if spec.reg_j else 0.0,
                    lambda3=lambdas[2] if spec.reg_aug else 0.0, nprobes=spec.nprobes, device="cuda:0",
                    sol_kwargs=dict(alg=pkg.Tsit5() if alg == 1 else pkg.RK4(), adaptive=False, nsteps=nsteps))


def mode_of(pkg, spec):
    return pkg.TestMode() if spec.mode == 2 else pkg.TrainMode(bool(spec.reg_z or spec.reg_j or spec.reg_aug))


def dev(a):
    return None if a is None else torch.tensor(np.asarray(a, dtype=np.float32), device="cuda:0")


def data_args(spec, xs, ys, p):
    return (dev(xs),) + ((dev(ys),) if spec.ncond else ()) + (dev(p), {})


def check_inference(pkg, o64, spec, icnf, p, xs, eps, ys, alg, nsteps):
    logp, (E, n, A), u1 = pkg.inference(icnf, mode_of(pkg, spec), *data_args(spec, xs, ys, p), eps=dev(eps), return_state=True)
    ref, (Er, nr, Ar), u1r = o64.inference_fixed(spec, p, xs, 0.0, 1.0, nsteps, alg, eps, ys)
    for got, want in ((logp, ref), (E, Er), (n, nr), (A, Ar), (u1, u1r)):
        err = np.max(np.abs(got.cpu().numpy() - want))
        assert err < TOL_SOLVE, err


# ---- 1. one dynamics call ----
@pytest.mark.parametrize("act", NEW)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_aug_f_of_each_new_activation(act, mode, pkg, o64):
    spec = spec_of(o64, 4, [32, 48], act, mode=mode, nprobes=2 if mode == 1 else 1, reg_z=mode != 2, reg_j=mode != 2)
    B = 200
    p, xs, eps, ys = o64.synth_inputs(spec, B, 11 + act, bias_scale=0.2)
    rng = np.random.default_rng(act)
    u = np.concatenate([xs, rng.standard_normal((spec.naug + 3, B)).astype(np.float32)], 0)
    ref = o64.aug_f(spec, p, u, 0.3, None if mode == 2 else eps, ys)
    for path in (0, 1, 3):
        icnf = make_icnf(pkg, spec, 1, 4, path=path)
        m = mode_of(pkg, spec)
        assert icnf.kernel_path(m) == (3 if path == 0 else path)
        du = pkg.augmented_f(icnf, m, dev(u), dev(p), 0.3, None if mode == 2 else dev(eps), None).cpu().numpy()
        err = np.max(np.abs(du - ref) / (1.0 + np.abs(ref)))
        assert err < TOL_CALL, (path, err)


# ---- 2. inference at every shape band where tanh / softplus take a fused family ----
def default_arch(nv):
    D = 2 * nv + 1
    return dict(nvars=nv, naug=nv + 1, hidden=[4 * (D + 1)] * 2, reg_z=True, reg_j=True, reg_aug=True)


BANDS = [
    (dict(nvars=8, hidden=[64, 64, 64]), 256, 3),          # D = 8, 3 x 64: cfg2's metric kernel for tanh
    (default_arch(1), 256, 3),                              # the default architecture: per-wave kernels for softplus
    (default_arch(12), 200, 2),                             # cooperative kernels for softplus
    (default_arch(20), 100, 2),                             # the dealt cooperative kernel for softplus
    (dict(nvars=32, hidden=[256, 256, 256]), 64, 2),        # cfg4: the cooperative kernel for tanh
]


@pytest.mark.parametrize("act", NEW)
@pytest.mark.parametrize("band", range(len(BANDS)))
def test_inference_at_the_fused_shape_bands_runs_layer_wise(act, band, pkg, o64):
    kw, B, nsteps = BANDS[band]
    kw = dict(kw)
    spec = spec_of(o64, kw.pop("nvars"), kw.pop("hidden"), act, **kw)
    p, xs, eps, ys = o64.synth_inputs(spec, B, 40 + band, bias_scale=0.2)
    for alg in (0, 1):
        icnf = make_icnf(pkg, spec, alg, nsteps)
        m = mode_of(pkg, spec)
        assert icnf.kernel_family(m) == "layered" and icnf.kernel_family(m, B=B, whole_solve=True) == "layered"
        assert icnf.grad_path(m, B=B, alg=alg) == 2
        check_inference(pkg, o64, spec, icnf, p, xs, eps, ys, alg, nsteps)


@pytest.mark.parametrize("case", ["mixed", "conditioned", "wide_simt", "forced_simt"])
def test_inference_other_chains(case, pkg, o64):
    if case == "mixed":
        spec, B, path, fam = spec_of(o64, 5, [48, 40, 56], [5, 1, 7]), 300, 0, "layered"
    elif case == "conditioned":
        spec, B, path, fam = spec_of(o64, 3, [32, 32], 7, naug=2, ncond=2, reg_z=True, reg_j=True, reg_aug=True), 300, 0, "layered"
    elif case == "wide_simt":
        spec, B, path, fam = spec_of(o64, 2, [520], 5), 24, 0, "simt"
    else:
        spec, B, path, fam = spec_of(o64, 3, [32, 32], 6), 100, 1, "simt"
    p, xs, eps, ys = o64.synth_inputs(spec, B, 17, bias_scale=0.2)
    for alg in (0, 1):
        icnf = make_icnf(pkg, spec, alg, 2, path=path)
        assert icnf.kernel_family(mode_of(pkg, spec)) == fam
        check_inference(pkg, o64, spec, icnf, p, xs, eps, ys, alg, 2)


def test_planar_layer_with_sigmoid(pkg, o64):
    nv, D = 2, 5
    n_in = D + 1
    rng = np.random.default_rng(5)
    u, w, b = rng.uniform(-0.7, 0.7, D), rng.uniform(-0.7, 0.7, n_in), rng.uniform(-0.3, 0.3, 1)
    ps = np.concatenate([u, w, b]).astype(np.float32)
    B = 64
    xs = rng.standard_normal((nv, B)).astype(np.float32)
    eps = rng.standard_normal((D, B)).astype(np.float32)
    spec = o64.Spec(nvars=nv, naug=nv + 1, widths=[n_in, 1, D], acts=[4, 0], reg_z=True, reg_j=True, reg_aug=True)
    p_dense = np.concatenate([w, b, u, np.zeros(D)]).astype(np.float32)
    ref = o64.inference_fixed(spec, p_dense, xs, 0.0, 1.0, 6, 1, eps)
    icnf = pkg.ICNF(nvariables=nv, nn=pkg.Chain(pkg.PlanarLayer(n_in, D, pkg.sigmoid)), steer_rate=0.0, device="cuda:0",
                    sol_kwargs=dict(alg=pkg.Tsit5(), adaptive=False, nsteps=6))
    m = pkg.TrainMode(True)
    assert icnf.kernel_family(m) == "layered"
    logp, (E, n, A) = pkg.inference(icnf, m, dev(xs), dev(ps), {}, eps=dev(eps))
    assert np.max(np.abs(logp.cpu().numpy() - ref[0])) < TOL_SOLVE
    for a_, b_ in zip((E, n, A), ref[1]):
        assert np.max(np.abs(a_.cpu().numpy() - b_)) < TOL_SOLVE


# ---- 3. loss and gradient, with the pre-activations kept and recomputed ----
GRAD_CASES = [
    # (spec_of args, kwargs, lambdas, B, alg, nsteps, whether act'' must matter)
    ((3, [32, 32], 5), dict(naug=2, reg_z=True, reg_j=True, reg_aug=True), (0.01, 0.02, 0.03), 120, 1, 2, True),   # swish, VJP, all regularisers
    ((4, [48, 40], 7), dict(mode=1, reg_j=True), (0.0, 0.05, 0.0), 100, 0, 2, True),                               # GELU, JVP with reg_j
    ((3, [24, 24], 4), dict(mode=2), (0.0, 0.0, 0.0), 100, 1, 2, False),                                          # sigmoid, TestMode
    ((3, [40, 24], 6), dict(reg_z=True, reg_j=True), (0.02, 0.03, 0.0), 100, 0, 3, False),                        # ELU, VJP
    ((4, [32, 48, 24], [7, 5, 5, 5]), dict(ncond=2), (0.0, 0.0, 0.0), 100, 1, 2, True),                           # swish output layer (sbar_kernel)
    ((2, [32, 32], 7), dict(mode=2), (0.0, 0.0, 0.0), 80, 0, 2, True),                                            # GELU, TestMode
]


@pytest.mark.parametrize("recompute", [False, True])
@pytest.mark.parametrize("case", range(len(GRAD_CASES)))
def test_loss_and_gradient_with_x(case, recompute, pkg, o64, monkeypatch):
    (nv, hidden, acts), kw, lam, B, alg, nsteps, dd_matters = GRAD_CASES[case]
    spec = spec_of(o64, nv, hidden, acts, **kw)
    p, xs, eps, ys = o64.synth_inputs(spec, B, 300 + case, bias_scale=0.2)
    L, gref, gxref = o64.loss_and_grad(spec, p, xs, 0.0, 1.0, nsteps, alg, eps, ys, lam, wrt_x=True)
    if recompute:
        setsw(pkg, monkeypatch, RECOMPUTE)
    icnf = make_icnf(pkg, spec, alg, nsteps, lambdas=lam)
    m = mode_of(pkg, spec)
    assert icnf.grad_path(m, B=B, alg=alg) == 2
    val, g, gx = pkg.loss_and_gradient(icnf, m, *data_args(spec, xs, ys, p), eps=dev(eps), wrt_x=True)
    g, gx = g.cpu().numpy().astype(np.float64), gx.cpu().numpy().astype(np.float64)
    assert abs(float(val) - L) < 1e-4 + 2e-6 * abs(L)
    tol_g = 5e-5 * np.abs(gref).max() + 1e-6
    assert np.max(np.abs(g - gref)) < tol_g, np.max(np.abs(g - gref)) / np.abs(gref).max()
    assert np.max(np.abs(gx - gxref)) < 5e-5 * np.abs(gxref).max() + 1e-7
    if dd_matters and not recompute:
        o64.zero_dd = True
        _, g0 = o64.loss_and_grad(spec, p, xs, 0.0, 1.0, nsteps, alg, eps, ys, lam)
        o64.zero_dd = False
        assert np.max(np.abs(g0 - gref)) > 2 * tol_g       # the act'' term is visible at this tolerance


def test_recomputed_and_kept_pre_activations_give_the_same_bits(pkg, o64, monkeypatch):
    spec = spec_of(o64, 4, [48, 40, 56], [7, 5, 1])
    p, xs, eps, ys = o64.synth_inputs(spec, 500, 8, bias_scale=0.2)
    out = []
    for env in ({}, RECOMPUTE):
        setsw(pkg, monkeypatch, env)
        icnf = make_icnf(pkg, spec, 1, 3)
        _, g, gx = pkg.loss_and_gradient(icnf, pkg.TrainMode(False), dev(xs), dev(p), {}, eps=dev(eps), wrt_x=True)
        out.append((g, gx))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


# ---- 4. the reference's default solver ----
def test_default_architecture_with_swish_under_the_adaptive_solvers(pkg, o64):
    spec = spec_of(o64, 1, [12, 12], 5, naug=2, reg_z=True, reg_j=True, reg_aug=True)
    lam = (0.01, 0.01, 0.01)
    B = 256
    p, xs, eps, ys = o64.synth_inputs(spec, B, 21, bias_scale=0.2)
    icnf = make_icnf(pkg, spec, 1, 1, lambdas=lam)
    icnf.sol_kwargs = dict(alg=pkg.VCABM(), reltol=1e-4, abstol=1e-4)
    m = pkg.TrainMode(True)
    val = float(pkg.loss(icnf, m, dev(xs), dev(p), {}, eps=dev(eps)))
    assert icnf.last_solve_stats["alg_used"] == "VCABM"
    u0 = np.concatenate([xs.astype(np.float64), np.zeros((spec.naug + 3, B))], 0)
    u1, _ = o64.integrate_vcabm(spec, p, u0, 0.0, 1.0, 1e-4, 1e-4, eps)
    D = spec.D
    logp = o64.std_normal_logpdf(u1[:D]) - u1[D]
    A = np.sqrt((u1[spec.nvars:D] ** 2).sum(0))
    ref = float(np.mean(-logp + lam[0] * u1[D + 1] + lam[1] * u1[D + 2] + lam[2] * A))
    assert abs(val - ref) < 1e-3 * (1 + abs(ref)), (val, ref)
    icnf.sol_kwargs = dict(alg=pkg.Tsit5(), reltol=1e-4, abstol=1e-4)
    gval, g, gx = pkg.loss_and_gradient(icnf, m, dev(xs), dev(p), {}, eps=dev(eps), wrt_x=True)
    tg = [float(t) for t in icnf.last_solve_stats["tgrid"]]
    assert len(tg) >= 2
    L, gref, gxref = o64.loss_and_grad(spec, p, xs, 0.0, 1.0, len(tg) - 1, 1, eps, None, lam, wrt_x=True, tgrid=tg)
    assert abs(float(gval) - L) < 1e-4 + 2e-6 * abs(L)
    assert np.max(np.abs(g.cpu().numpy() - gref)) < 5e-5 * np.abs(gref).max() + 1e-6
    assert np.max(np.abs(gx.cpu().numpy() - gxref)) < 5e-5 * np.abs(gxref).max() + 1e-7


# ---- 5. generate ----
@pytest.mark.parametrize("act", [4, 6])
def test_generate_over_the_reversed_tspan(act, pkg, o64):
    spec = spec_of(o64, 3, [32, 32], act)
    B = 128
    p, _, eps, ys = o64.synth_inputs(spec, B, 60 + act, bias_scale=0.2)
    z0 = np.random.default_rng(act).standard_normal((spec.D, B)).astype(np.float32)
    icnf = make_icnf(pkg, spec, 1, 4)
    x = pkg.generate(icnf, pkg.TrainMode(False), dev(p), {}, B, z0=dev(z0), eps=dev(eps))
    u0 = np.concatenate([z0.astype(np.float64), np.zeros((3, B))], 0)
    ref = o64.integrate_fixed(spec, p, u0, 1.0, 0.0, 4, 1, eps, ys)
    assert np.max(np.abs(x.cpu().numpy() - ref[:spec.nvars])) < TOL_SOLVE


# ---- 6. saturation ----
@pytest.mark.parametrize("act", NEW)
def test_saturated_pre_activations_stay_finite_and_exact(act, pkg, o64):
    spec = spec_of(o64, 3, [32, 32], act, reg_z=True, reg_j=True)
    B, nsteps, lam, t1 = 128, 2, (0.01, 0.01, 0.0), 0.05
    p, xs, eps, ys = o64.synth_inputs(spec, B, 90 + act, bias_scale=0.2)
    w_off, b_off, _ = spec.param_offsets()
    p = p.copy()
    p[w_off[0]:b_off[0] + spec.widths[1]] *= 30.0                   # first layer: pre-activations up to |a| ~ 60
    layers = o64.unpack_params(spec, p)
    zin = np.concatenate([xs, np.zeros((1, B))], 0)
    a1 = layers[0][0].numpy() @ zin + layers[0][1].numpy()[:, None]
    assert np.abs(a1).max() > 50
    icnf = make_icnf(pkg, spec, 1, nsteps, lambdas=lam, tspan=(0.0, t1))
    m = mode_of(pkg, spec)
    logp, (E, n, A), u1 = pkg.inference(icnf, m, dev(xs), dev(p), {}, eps=dev(eps), return_state=True)
    ref, (Er, nr, _), u1r = o64.inference_fixed(spec, p, xs, 0.0, t1, nsteps, 1, eps)
    for got, want in ((logp, ref), (E, Er), (n, nr), (u1, u1r)):
        got = got.cpu().numpy()
        assert np.all(np.isfinite(got))
        assert np.max(np.abs(got - want)) < TOL_SOLVE * max(1.0, np.abs(want).max())
    val, g, gx = pkg.loss_and_gradient(icnf, m, dev(xs), dev(p), {}, eps=dev(eps), wrt_x=True)
    L, gref, gxref = o64.loss_and_grad(spec, p, xs, 0.0, t1, nsteps, 1, eps, None, lam, wrt_x=True)
    g, gx = g.cpu().numpy(), gx.cpu().numpy()
    assert np.all(np.isfinite(g)) and np.all(np.isfinite(gx))
    assert abs(float(val) - L) < 1e-4 + 2e-6 * abs(L)
    assert np.max(np.abs(g - gref)) < 5e-5 * np.abs(gref).max() + 1e-6
    assert np.max(np.abs(gx - gxref)) < 5e-5 * np.abs(gxref).max() + 1e-7


# ---- 7. the C ABI ----
def test_cnf_create_accepts_exactly_the_enum(pkg):
    lib = pkg._lib.load()

    def create(acts, arith=0, path=0):
        cfg = pkg._lib.CnfConfig()
        cfg.nvars, cfg.naug, cfg.ncond, cfg.autonomous, cfg.n_layers = 4, 0, 0, 0, 3
        for i, w in enumerate((5, 32, 32, 4)):
            cfg.widths[i] = w
        for i, a in enumerate(acts):
            cfg.acts[i] = a
        cfg.mode, cfg.nprobes, cfg.kernel_path, cfg.arith = 0, 1, path, arith
        h = C.c_void_p()
        rc = lib.cnf_create(C.byref(h), C.byref(cfg))
        if rc == 0:
            lib.cnf_destroy(h)
        return rc

    for a in (0, 1, 2, 4, 5, 6, 7):
        assert create([a, a, 0]) == 0
        assert create([a, 1, a]) == 0
    for a in (3, 8, -1, 100):
        assert create([a, 1, 0]) == pkg._lib.ERR_INVALID
        assert create([1, 1, a]) == pkg._lib.ERR_INVALID
    for a in NEW:
        assert create([a, a, 0], arith=pkg._lib.ARITH_BF16X6) == pkg._lib.ERR_UNSUPPORTED
        assert create([a, a, 0], path=2) == pkg._lib.ERR_UNSUPPORTED                 # no fused instance
