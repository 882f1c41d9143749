"""CPU: the cotangent of the conditions (cnf_integrate_fixed_vjp_cond / cnf_integrate_grid_vjp_cond, include/cnf.h) - the fp64
reference the GPU tests rest on (tests/cond_vjp_reference.py) is checked against central differences of its own solve and against
vjp_reference.py on everything the two share; the new entries validate their arguments without a device and the Python layer
refuses on the arguments alone."""
import numpy as np
import pytest
import torch

import cond_vjp_reference as cref
import vjp_reference as ref

TOL64 = 1e-9    # test_vjp_host.py's bound between two float64 evaluations of the same formulas
FD_H = 1e-6     # central differences in float64: truncation ~ h^2, rounding ~ 1e-16 / h
FD_TOL = 1e-7   # of max|ys_bar|

# (nvars, hidden, act, spec keywords, alg, nsteps, B)
CASES = {
    "conditioned RNODE, VJP mode": (2, [32, 32], 1, dict(ncond=3, reg_z=True, reg_j=True), 1, 2, 5),
    "exact trace": (3, [16, 16], 1, dict(ncond=2, mode=2), 1, 2, 4),
    "JVP, two probes, autonomous, softplus": (2, [16, 16], 2, dict(ncond=2, mode=1, nprobes=2, autonomous=True), 0, 3, 4),
}
_cache = {}


def case(o64, name):
    """Inputs and the helper's pullback of one case, computed once and shared (read-only) by the tests below."""
    if name not in _cache:
        nvars, hidden, act, kw, alg, nsteps, B = CASES[name]
        spec = o64.make_spec(nvars, hidden, act=act, **kw)
        p, xs, eps, ys = o64.synth_inputs(spec, B, seed=41, bias_scale=0.2)
        rng = np.random.default_rng(7)
        u0 = np.concatenate([xs, 0.5 * rng.standard_normal((spec.naug + 3, B))], 0).astype(np.float64)
        bar = rng.standard_normal((spec.D + 3, B))
        out = cref.pullback(o64, spec, p, u0, ys, bar, 0.0, 1.0, nsteps, alg, eps)
        _cache[name] = (spec, p, u0, eps, ys.astype(np.float64), bar, alg, nsteps, out)
    return _cache[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_ys_bar_against_central_differences(name, oracles):
    o64, _ = oracles
    spec, p, u0, eps, ys, bar, alg, nsteps, (_, _, ys_bar, _) = case(o64, name)

    def column_scalars(y):   # L_j = <u1_bar[:, j], u1[:, j]>: columns are independent, so one row of ys is perturbed in all of them at once
        u1 = cref.integrate(o64, spec, p, u0, y, 0.0, 1.0, nsteps, alg, eps).detach().numpy()
        return (u1 * bar).sum(0)

    fd = np.zeros_like(ys_bar)
    for c in range(spec.ncond):
        yp, ym = ys.copy(), ys.copy()
        yp[c] += FD_H
        ym[c] -= FD_H
        fd[c] = (column_scalars(yp) - column_scalars(ym)) / (2 * FD_H)
    err, scale = np.abs(fd - ys_bar).max(), np.abs(ys_bar).max()
    print(f"{name}: ys_bar vs central differences {err:.3e}, max|ys_bar| {scale:.3e}")
    assert scale > 1e-2
    assert err <= FD_TOL * scale


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_agrees_with_vjp_reference_on_what_they_share(name, oracles):
    o64, _ = oracles
    spec, p, u0, eps, ys, bar, alg, nsteps, (gp, gu, _, u1) = case(o64, name)
    gp0, gu0, u10 = ref.pullback(o64, spec, p, u0, bar, 0.0, 1.0, nsteps, alg, eps, ys)
    assert np.abs(u1 - u10).max() <= TOL64 * np.abs(u10).max()
    assert np.abs(gp - gp0).max() <= TOL64 * np.abs(gp0).max()
    assert np.abs(gu - gu0).max() <= TOL64 * np.abs(gu0).max()


def test_null_and_inconsistent_arguments_are_errors_not_crashes(pkg):
    lib = pkg._lib.load()
    INV = pkg._lib.ERR_INVALID
    assert lib.cnf_integrate_fixed_vjp_cond(None, 1, 4, 0.0, 1.0, None, None, None, 4, None, None, None, None, None, None) == INV
    assert "null handle" in lib.cnf_last_error().decode()
    assert lib.cnf_integrate_fixed_vjp_cond(None, 1, 0, 0.0, 1.0, None, None, None, 4, None, None, None, None, None, None) == INV   # no steps
    grid = (pkg._lib.C.c_float * 3)(0.0, 0.5, 1.0)
    assert lib.cnf_integrate_grid_vjp_cond(None, 1, 2, grid, None, None, None, 4, None, None, None, None, None, None) == INV
    assert lib.cnf_integrate_grid_vjp_cond(None, 1, 2, None, None, None, None, 4, None, None, None, None, None, None) == INV      # no grid
    assert "cnf_integrate_grid_vjp_cond" in lib.cnf_last_error().decode()
    assert lib.cnf_integrate_grid_vjp_cond(None, 1, 0, grid, None, None, None, 4, None, None, None, None, None, None) == INV      # no steps
    for name in ("cnf_integrate_fixed_vjp_cond", "cnf_integrate_grid_vjp_cond"):
        assert name in pkg._lib.EXPORTS


def test_cond_grad_argument_errors_come_before_any_library_call(pkg):
    """No device here: reaching the library would raise CnfError (no CPU fallback), so these exceptions show the refusal is made
    on the arguments alone."""
    fixed = dict(alg=pkg.Tsit5(), adaptive=False, nsteps=4)
    nn = pkg.Chain(pkg.Dense(3, 8, pkg.tanh), pkg.Dense(8, 2))
    xs, ps = torch.zeros(2, 4), torch.zeros(nn.param_offsets()[2])
    plain = pkg.ICNF(nvariables=2, naugments=0, nn=nn, sol_kwargs=fixed)
    with pytest.raises(ValueError, match="no conditions"):
        pkg.inference(plain, pkg.TrainMode(), xs, ps, {}, differentiable=True, cond_grad=True)
    with pytest.raises(ValueError, match="no conditions"):
        pkg.generate(plain, pkg.TrainMode(), ps, {}, 4, differentiable=True, cond_grad=True)
    with pytest.raises(ValueError, match="no conditions"):
        pkg.integrate_vjp(plain, pkg.TrainMode(), torch.zeros(5, 4), ps, torch.zeros(5, 4), t0=0.0, t1=1.0, eps=None, want_ys_bar=True)
    nnc = pkg.Chain(pkg.Dense(4, 8, pkg.tanh), pkg.Dense(8, 2))
    psc = torch.zeros(nnc.param_offsets()[2])
    ys = torch.zeros(1, 4, requires_grad=True)
    cond = pkg.ICNF(nvariables=2, naugments=0, nconditions=1, nn=nnc, sol_kwargs=fixed)
    with pytest.raises(ValueError, match="differentiable=True"):
        pkg.inference(cond, pkg.TrainMode(), xs, ys, psc, {}, cond_grad=True)
    with pytest.raises(ValueError, match="differentiable=True"):
        pkg.generate(cond, pkg.TrainMode(), ys, psc, {}, 4, cond_grad=True)
    with pytest.raises(NotImplementedError, match="cond_grad=True"):      # the refusal without cond_grad stands and points to it
        pkg.inference(cond, pkg.TrainMode(), xs, ys, psc, {}, differentiable=True)
    vc = pkg.ICNF(nvariables=2, naugments=0, nconditions=1, nn=nnc)      # the reference's default solver: VCABM
    with pytest.raises(NotImplementedError, match="Tsit5"):
        pkg.inference(vc, pkg.TrainMode(), xs, ys, psc, {}, differentiable=True, cond_grad=True)
    with pytest.raises(NotImplementedError, match="Tsit5"):
        pkg.generate(vc, pkg.TrainMode(), ys, psc, {}, 4, differentiable=True, cond_grad=True)
