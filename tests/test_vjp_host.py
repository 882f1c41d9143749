"""CPU: the pullback of the solve (cnf_integrate_fixed_vjp / cnf_integrate_grid_vjp, include/cnf.h) - the fp64 reference the GPU
tests rest on is checked against the committed oracle, and the new entries validate their arguments without a device."""
import numpy as np
import pytest
import torch

import vjp_reference as ref

# Both sides are float64 evaluations of the same formulas (the difference measured when this was written is <= 9e-16 relative);
# 1e-9 still sits four orders below the float32 tolerance this reference underpins.
TOL64 = 1e-9

# (nvars, hidden, act, spec keywords, lambdas, alg, nsteps, B)
CONFIGS = {
    "3x64 tanh, Tsit5": (8, [64, 64, 64], 1, dict(), (0.0, 0.0, 0.0), 1, 3, 6),
    "RNODE with naug, all regularisers, RK4": (3, [24, 24], 1, dict(naug=2, reg_z=True, reg_j=True, reg_aug=True), (0.01, 0.02, 0.03), 0, 4, 5),
    "default net at nvariables = 1": (1, [16, 16], 2, dict(naug=2, reg_z=True, reg_j=True), (0.01, 0.01, 0.0), 1, 3, 7),
    "conditioned RNODE": (2, [32, 32], 1, dict(ncond=3, reg_z=True, reg_j=True), (0.05, 0.02, 0.0), 1, 2, 5),
    "conditioned, no l3": (2, [16, 16], 2, dict(ncond=2, naug=1, reg_aug=False), (0.0, 0.0, 0.0), 0, 3, 4),
    "exact trace": (3, [16, 16], 1, dict(mode=2), (0.0, 0.0, 0.0), 1, 2, 4),
    "JVP with reg_z": (3, [16, 16], 2, dict(mode=1, reg_z=True), (0.04, 0.0, 0.0), 0, 3, 5),
    "JVP, two probes, l3": (2, [16, 16], 1, dict(mode=1, nprobes=2, naug=2, reg_aug=True), (0.0, 0.0, 0.1), 1, 2, 4),
}


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_reference_reproduces_the_oracle(name, oracles):
    o64, _ = oracles
    nvars, hidden, act, kw, lambdas, alg, nsteps, B = CONFIGS[name]
    spec = o64.make_spec(nvars, hidden, act=act, **kw)
    p, xs, eps, ys = o64.synth_inputs(spec, B, seed=31, bias_scale=0.2)
    u0 = np.concatenate([xs.astype(np.float64), np.zeros((spec.naug + 3, B))], 0)
    # forward values: the oracle's own solve
    want = o64.integrate_fixed(spec, p, u0, 0.0, 1.0, nsteps, alg, eps, ys)
    got = ref.integrate(o64, spec, p, u0, 0.0, 1.0, nsteps, alg, eps, ys).detach().numpy()
    err = np.abs(got - want).max()
    print(f"{name}: values {err:.3e} of {np.abs(want).max():.3e}")
    assert err <= TOL64 * np.abs(want).max()
    # with the loss's own cotangent the pullback is the oracle's gradient of the loss, with respect to the data too
    L, gp, gx = o64.loss_and_grad(spec, p, xs, 0.0, 1.0, nsteps, alg, eps, ys, lambdas=lambdas, wrt_x=True)
    bar = ref.loss_cotangent(spec, want, lambdas, B)
    grad, u0_bar, u1 = ref.pullback(o64, spec, p, u0, bar, 0.0, 1.0, nsteps, alg, eps, ys)
    eg, ex = np.abs(grad - gp).max(), np.abs(u0_bar[:nvars] - gx).max()
    print(f"{name}: grad {eg:.3e} of {np.abs(gp).max():.3e}; grad_x {ex:.3e} of {np.abs(gx).max():.3e}")
    assert eg <= TOL64 * np.abs(gp).max()
    assert ex <= TOL64 * np.abs(gx).max()
    D = spec.D
    assert np.array_equal(u0_bar[D:], bar[D:])           # the dlogp / E / n rows feed nothing: passed through
    assert np.abs(u1 - want).max() <= TOL64 * np.abs(want).max()


def test_reference_on_a_grid_and_backwards(oracles):
    """A non-uniform grid reproduces the oracle's frozen-grid gradient; a reversed span is the solve `generate` runs."""
    o64, _ = oracles
    spec = o64.make_spec(4, [16, 16], act=1, reg_z=True, reg_j=True)
    B, lambdas = 5, (0.02, 0.03, 0.0)
    p, xs, eps, ys = o64.synth_inputs(spec, B, seed=5, bias_scale=0.2)
    u0 = np.concatenate([xs.astype(np.float64), np.zeros((3, B))], 0)
    grid = [0.0, 0.1, 0.35, 0.7, 1.0]
    L, gp, gx = o64.loss_and_grad(spec, p, xs, 0.0, 1.0, 4, 1, eps, ys, lambdas=lambdas, wrt_x=True, tgrid=grid)
    u1 = ref.integrate(o64, spec, p, u0, 0.0, 1.0, None, 1, eps, ys, tgrid=grid).detach().numpy()
    grad, u0_bar, _ = ref.pullback(o64, spec, p, u0, ref.loss_cotangent(spec, u1, lambdas, B), 0.0, 1.0, None, 1, eps, ys, tgrid=grid)
    assert np.abs(grad - gp).max() <= TOL64 * np.abs(gp).max()
    assert np.abs(u0_bar[:4] - gx).max() <= TOL64 * np.abs(gx).max()
    back = o64.integrate_fixed(spec, p, u1, 1.0, 0.0, 4, 1, eps, ys)
    got = ref.integrate(o64, spec, p, u1, 1.0, 0.0, 4, 1, eps, ys).detach().numpy()
    assert np.abs(got - back).max() <= TOL64 * np.abs(back).max()


def test_reference_activation_table_matches_the_oracles(oracles):
    o64, _ = oracles
    a = torch.linspace(-4, 4, 41, dtype=torch.float64)
    for kind in (0, 1, 2):
        assert torch.equal(ref.act(a, kind), o64._act(a, kind))
    for kind in (4, 5, 6, 7):
        assert torch.isfinite(ref.act(a, kind)).all()


def test_null_and_inconsistent_arguments_are_errors_not_crashes(pkg):
    lib = pkg._lib.load()
    INV = pkg._lib.ERR_INVALID
    assert lib.cnf_integrate_fixed_vjp(None, 1, 4, 0.0, 1.0, None, None, None, 4, None, None, None, None, None) == INV
    assert "null handle" in lib.cnf_last_error().decode()
    grid = (pkg._lib.C.c_float * 3)(0.0, 0.5, 1.0)
    assert lib.cnf_integrate_grid_vjp(None, 1, 2, grid, None, None, None, 4, None, None, None, None, None) == INV
    assert lib.cnf_integrate_grid_vjp(None, 1, 2, None, None, None, None, 4, None, None, None, None, None) == INV     # no grid
    assert "cnf_integrate_grid_vjp" in lib.cnf_last_error().decode()
    assert lib.cnf_integrate_grid_vjp(None, 1, 0, grid, None, None, None, 4, None, None, None, None, None) == INV     # no steps
    assert lib.cnf_vjp_path_for(None, 4, 1, 0) == INV
    for name in ("cnf_integrate_fixed_vjp", "cnf_integrate_grid_vjp", "cnf_vjp_path_for"):
        assert name in pkg._lib.EXPORTS


def test_differentiable_argument_errors_come_before_any_library_call(pkg):
    """No device here: reaching the library would raise CnfError (no CPU fallback), so NotImplementedError shows the refusal is
    made on the arguments alone."""
    nn = pkg.Chain(pkg.Dense(3, 8, pkg.tanh), pkg.Dense(8, 2))
    xs, ps = torch.zeros(2, 4), torch.zeros(nn.param_offsets()[2])
    vc = pkg.ICNF(nvariables=2, naugments=0, nn=nn)                      # the reference's default solver: VCABM
    with pytest.raises(NotImplementedError, match="Tsit5"):
        pkg.inference(vc, pkg.TrainMode(), xs, ps, {}, differentiable=True)
    with pytest.raises(NotImplementedError, match="Tsit5"):
        pkg.generate(vc, pkg.TrainMode(), ps, {}, 4, differentiable=True)
    with pytest.raises(NotImplementedError, match="Tsit5"):
        pkg.integrate_vjp(vc, pkg.TrainMode(), torch.zeros(5, 4), ps, torch.zeros(5, 4), t0=0.0, t1=1.0, eps=None)
    nnc = pkg.Chain(pkg.Dense(4, 8, pkg.tanh), pkg.Dense(8, 2))
    cond = pkg.ICNF(nvariables=2, naugments=0, nconditions=1, nn=nnc, sol_kwargs=dict(alg=pkg.Tsit5(), adaptive=False, nsteps=4))
    ys = torch.zeros(1, 4, requires_grad=True)
    with pytest.raises(NotImplementedError, match="detach"):
        pkg.inference(cond, pkg.TrainMode(), xs, ys, torch.zeros(nnc.param_offsets()[2]), {}, differentiable=True)
