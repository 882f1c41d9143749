"""CPU: Float64 flows (ICNF(data_type=torch.float64), include/cnf.h cnf_*_f64) - what can be checked without a device.  There is
no CPU fallback, so reaching the library raises CnfError: a NotImplementedError / TypeError here shows the refusal was made on the
arguments alone, before any library call (the pattern of tests/test_vjp_host.py)."""
import os
import re

import pytest
import torch

from conftest import ROOT

F64_ENTRIES = ("cnf_f64_supported", "cnf_set_params_f64", "cnf_aug_f_f64", "cnf_integrate_fixed_f64", "cnf_inference_fixed_f64")


def flow(pkg, dtype=torch.float64, **kw):
    nn = pkg.Chain(pkg.Dense(3, 8, pkg.tanh), pkg.Dense(8, 2))
    kw.setdefault("sol_kwargs", dict(alg=pkg.Tsit5(), adaptive=False, nsteps=4))
    return pkg.ICNF(data_type=dtype, nvariables=2, naugments=0, nn=nn, **kw), nn


def test_constructor_accepts_float64(pkg):
    icnf, _ = flow(pkg)
    assert icnf.data_type is torch.float64 and icnf.f64
    d = pkg.ICNF(data_type=torch.float64, nvariables=1)          # the default architecture
    assert d.f64 and d.nn.widths == [4, 16, 16, 3]


def test_float32_constructor_path_is_unchanged(pkg):
    icnf, _ = flow(pkg, torch.float32)
    assert icnf.data_type is torch.float32 and not icnf.f64
    assert pkg.ICNF(nvariables=1).data_type is torch.float32     # the default
    for bad in (torch.float16, torch.bfloat16, torch.int32, None):
        with pytest.raises(TypeError, match="Float32"):
            pkg.ICNF(data_type=bad, nvariables=1)
    ps, st = pkg.setup(torch.Generator().manual_seed(3), icnf)
    assert ps.dtype == torch.float32 and st == {}


@pytest.mark.parametrize("planar", [False, True])
def test_setup_returns_float64_in_the_float32_layout(pkg, planar):
    def build(dtype):
        nn = pkg.Chain(pkg.PlanarLayer(3, 2, pkg.tanh)) if planar else pkg.Chain(pkg.Dense(3, 8, pkg.tanh), pkg.Dense(8, 2))
        return pkg.ICNF(data_type=dtype, nvariables=2, naugments=0, nn=nn)
    i64, i32 = build(torch.float64), build(torch.float32)
    p64, _ = pkg.setup(torch.Generator().manual_seed(7), i64)
    p32, _ = pkg.setup(torch.Generator().manual_seed(7), i32)
    assert p64.dtype == torch.float64 and p32.dtype == torch.float32
    assert i64.nn.param_offsets() == i32.nn.param_offsets() and p64.numel() == i64.nn.param_offsets()[2]
    assert torch.equal(p64.to(torch.float32), p32)               # the same draw, rounded: same layout, same offsets
    assert not torch.equal(p64, p32.to(torch.float64))           # and genuinely double


def test_refusals_name_float32_and_come_before_any_library_call(pkg):
    xs = torch.zeros(2, 4, dtype=torch.float64)
    fixed, nn = flow(pkg)
    ps = torch.zeros(nn.param_offsets()[2], dtype=torch.float64)
    train = pkg.TrainMode()
    # adaptive stepping and VCABM
    default, _ = flow(pkg, sol_kwargs={})                                              # the reference's default: VCABM
    adaptive, _ = flow(pkg, sol_kwargs=dict(alg=pkg.Tsit5()))                          # adaptive unless adaptive=False
    vcabm, _ = flow(pkg, sol_kwargs=dict(alg=pkg.VCABM(), reltol=1e-6))
    for icnf in (default, adaptive, vcabm):
        with pytest.raises(NotImplementedError, match="Float32"):
            pkg.inference(icnf, train, xs, ps, {})
        with pytest.raises(NotImplementedError, match="Float32"):
            pkg.generate(icnf, train, ps, {}, 4)
        with pytest.raises(NotImplementedError, match="Float32"):
            pkg.loss(icnf, train, xs, ps, {})
    # gradients
    with pytest.raises(NotImplementedError, match="Float32"):
        pkg.loss_and_gradient(fixed, train, xs, ps, {})
    with pytest.raises(NotImplementedError, match="Float32"):
        pkg.inference(fixed, train, xs, ps, {}, differentiable=True)
    with pytest.raises(NotImplementedError, match="Float32"):
        pkg.generate(fixed, train, ps, {}, 4, differentiable=True)
    with pytest.raises(NotImplementedError, match="Float32"):
        pkg.integrate_vjp(fixed, train, torch.zeros(5, 4, dtype=torch.float64), ps, torch.zeros(5, 4, dtype=torch.float64),
                          t0=0.0, t1=1.0, eps=None)
    # fit
    with pytest.raises(NotImplementedError, match="Float32"):
        pkg.ICNFModel(icnf=fixed, epochs=1).fit(torch.zeros(8, 2))
    cond = pkg.ICNF(data_type=torch.float64, nvariables=2, naugments=0, nconditions=1,
                    nn=pkg.Chain(pkg.Dense(4, 8, pkg.tanh), pkg.Dense(8, 2)), sol_kwargs=dict(alg=pkg.RK4(), adaptive=False, nsteps=2))
    with pytest.raises(NotImplementedError, match="Float32"):
        pkg.CondICNFModel(icnf=cond, epochs=1).fit((torch.zeros(8, 2), torch.zeros(8, 1)))


def test_a_float32_tensor_given_to_a_float64_flow_is_a_type_error_not_a_cast(pkg):
    icnf, nn = flow(pkg)
    n = nn.param_offsets()[2]
    x64, x32 = torch.zeros(2, 4, dtype=torch.float64), torch.zeros(2, 4)
    p64, p32 = torch.zeros(n, dtype=torch.float64), torch.zeros(n)
    train = pkg.TrainMode()
    with pytest.raises(TypeError, match="float32"):
        pkg.inference(icnf, train, x32, p64, {})
    with pytest.raises(TypeError, match="float32"):
        pkg.inference(icnf, train, x64, p32, {})
    with pytest.raises(TypeError, match="float32"):
        pkg.loss(icnf, train, x32, p64, {})
    with pytest.raises(TypeError, match="float32"):
        pkg.generate(icnf, train, p32, {}, 4)
    with pytest.raises(TypeError, match="float32"):
        pkg.generate(icnf, train, p64, {}, 4, z0=x32)
    with pytest.raises(TypeError, match="float32"):
        pkg.augmented_f(icnf, train, torch.zeros(5, 4), p64, 0.0, None)
    with pytest.raises(TypeError, match="float32"):
        pkg.ICNFDist(icnf, pkg.TestMode(), p64, {}).logpdf(x32)
    # with everything in double the call passes the precision checks: the next complaint is about where these host tensors live
    with pytest.raises(ValueError, match="must live on"):
        pkg.inference(icnf, train, x64, p64, {})


def test_the_plan_of_a_fixed_dt_solve_is_the_float32_entries_plan(pkg):
    """dt with a shorter last step: full steps and the tail as two spans of equal steps, on the grid fixed_dt_grid computes."""
    from cnf_amd import icnf as m
    tail, _ = flow(pkg, sol_kwargs=dict(alg=pkg.Tsit5(), adaptive=False, dt=0.3))
    spans = m._f64_spans(tail, 0.0, 1.0)
    grid = tail.fixed_dt_grid(0.0, 1.0, tail._fixed_dt())
    assert len(grid) == 5 and spans == [(grid[0], grid[3], 3), (grid[3], grid[4], 1)]
    back = m._f64_spans(tail, 1.0, 0.0)
    assert [n for _, _, n in back] == [3, 1] and back[0][0] == 1.0 and back[1][1] == 0.0
    even, _ = flow(pkg, sol_kwargs=dict(alg=pkg.RK4(), adaptive=False, dt=0.25))
    assert m._f64_spans(even, 0.0, 1.0) == [(0.0, 1.0, 4)]
    steps, _ = flow(pkg)
    assert m._f64_spans(steps, 0.0, 1.0) == [(0.0, 1.0, 4)]


def test_the_abi_declares_and_exports_the_five_entries(pkg):
    text = open(os.path.join(ROOT, "include", "cnf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = pkg._lib.load()
    for name in F64_ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert name in pkg._lib.EXPORTS and hasattr(lib, name)
    # null arguments are errors, not crashes
    INV = pkg._lib.ERR_INVALID
    assert lib.cnf_f64_supported(None) == 0 and "null handle" in lib.cnf_last_error().decode()
    assert lib.cnf_set_params_f64(None, None, 0, None, None, 0, None) == INV
    assert lib.cnf_aug_f_f64(None, None, None, 0.0, None, None, 4, None) == INV
    assert lib.cnf_integrate_fixed_f64(None, 1, 4, 0.0, 1.0, None, None, None, 4, None, None) == INV
    assert lib.cnf_inference_fixed_f64(None, 1, 4, 0.0, 1.0, None, None, None, 4, None, None, None, None) == INV
    assert "cnf_inference_fixed_f64" in lib.cnf_last_error().decode()
