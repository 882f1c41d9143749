"""Sigmoid, swish, ELU and GELU hidden layers (include/cnf.h CNF_ACT_SIGMOID .. CNF_ACT_GELU): the host side.  The ids every
front end maps, and the closed forms of act' and act'' that the kernels implement (csrc/cnf_common.h: act_fwd_rt, act_dd_rt),
restated in fp64 and checked against torch's double backward."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_IDS = {"sigmoid": 4, "swish": 5, "elu": 6, "gelu": 7}


def header_enum():
    with open(os.path.join(ROOT, "include", "cnf.h")) as f:
        text = f.read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"\bCNF_ACT_([A-Z]+)\s*=\s*(\d+)", text)}


def test_dense_maps_names_functions_and_torch_aliases(pkg):
    for name, i in NEW_IDS.items():
        assert pkg.Dense(4, 8, name).act_id == i
        assert pkg.Dense(4, 8, getattr(pkg, name)).act_id == i
    assert pkg.Dense(4, 8, torch.sigmoid).act_id == 4
    assert pkg.Dense(4, 8, torch.nn.functional.silu).act_id == 5
    assert pkg.Dense(4, 8, "silu").act_id == 5
    for act in (torch.relu, "relu", torch.nn.functional.gelu):
        with pytest.raises(TypeError, match="MethodError"):
            pkg.Dense(4, 8, act).act_id


def test_module_functions_compute_the_activations(pkg):
    a = torch.linspace(-6, 6, 101, dtype=torch.float64)
    assert torch.allclose(pkg.sigmoid(a), 1 / (1 + torch.exp(-a)))
    assert torch.allclose(pkg.swish(a), a / (1 + torch.exp(-a)))
    assert torch.allclose(pkg.elu(a), torch.where(a >= 0, a, torch.expm1(a)))
    k = np.sqrt(2 / np.pi)
    assert torch.allclose(pkg.gelu(a), a / 2 * (1 + torch.tanh(k * (a + 0.044715 * a ** 3))))


def test_icnf_with_new_activations_constructs_and_the_default_net_is_unchanged(pkg):
    for act in (pkg.swish, pkg.gelu):
        icnf = pkg.ICNF(nvariables=2, naugments=0, nn=pkg.Chain(pkg.Dense(3, 16, act), pkg.Dense(16, 16, pkg.tanh), pkg.Dense(16, 2)))
        assert [l.act_id for l in icnf.nn.layers] == [NEW_IDS[act.__name__], 1, 0]
    icnf = pkg.ICNF(nvariables=3)
    assert [l.act_id for l in icnf.nn.layers] == [2, 2, 0]
    pl = pkg.PlanarLayer(3, 2, pkg.sigmoid)
    icnf = pkg.ICNF(nvariables=2, naugments=0, nn=pkg.Chain(pl))
    assert [l.act_id for l in icnf.nn.layers] == [4, 0]


def test_header_enum_matches_the_python_constants(pkg):
    enum = header_enum()
    lib = pkg._lib
    assert enum == {"IDENTITY": lib.ACT_IDENTITY, "TANH": lib.ACT_TANH, "SOFTPLUS": lib.ACT_SOFTPLUS, "SIGMOID": lib.ACT_SIGMOID,
                    "SWISH": lib.ACT_SWISH, "ELU": lib.ACT_ELU, "GELU": lib.ACT_GELU}
    assert 3 not in enum.values()
    assert {k.lower(): v for k, v in enum.items() if v >= 4} == NEW_IDS


def test_julia_act_id_methods_match_the_header():
    with open(os.path.join(ROOT, "julia", "hip_ext", "handle.jl")) as f:
        text = f.read()
    methods = {m.group(1): int(m.group(2)) for m in re.finditer(r"act_id\(::typeof\(([\w.]+)\)\)\s*=\s*Int32\((\d+)\)", text)}
    enum = header_enum()
    expect = {"identity": enum["IDENTITY"], "tanh": enum["TANH"], "NNlib.tanh_fast": enum["TANH"], "NNlib.softplus": enum["SOFTPLUS"],
              "NNlib.sigmoid": enum["SIGMOID"], "NNlib.sigmoid_fast": enum["SIGMOID"], "NNlib.swish": enum["SWISH"],
              "NNlib.elu": enum["ELU"], "NNlib.gelu": enum["GELU"]}
    assert methods == expect
    assert "sigmoid, swish, elu, gelu" in text


# ---- the kernels' closed forms (csrc/cnf_common.h), restated in numpy fp64 ----
def _sig_pair(x):
    e = np.exp(-np.abs(x))
    one = np.ones_like(x)
    r = one / (one + e)
    p = e * r
    return np.where(x >= 0, r, p), np.where(x >= 0, p, r)


K0, K1 = 0.7978845608028654, 0.7978845608028654 * 0.044715


def _gelu_tail(a):
    return np.where(np.abs(a) > 1e4, np.copysign(np.asarray(1e4, a.dtype), a), a)


def closed_forms(act, a):
    """(h, act', act'') as act_fwd_rt / act_dd_rt compute them; act_dd_rt's x is h (sigmoid, ELU) or a (swish, GELU)."""
    if act == "sigmoid":
        s, c = _sig_pair(a)
        h, d = s, s * c
        return h, d, d * (1.0 - 2.0 * h)
    if act == "swish":
        s, c = _sig_pair(a)
        h = a * s
        d = h * c + s
        return h, d, s * c * (a * (c - s) + 2.0)
    if act == "elu":
        e = np.exp(np.minimum(a, 0.0))
        h = np.where(a >= 0, a, np.expm1(np.minimum(a, 0.0)))
        d = np.where(a >= 0, 1.0, e)
        return h, d, np.where(h < 0, d, 0.0)
    if act == "gelu":
        t = _gelu_tail(a)
        t2 = t * t
        s, c = _sig_pair(2.0 * t * (K1 * t2 + K0))
        du = 3.0 * K1 * t2 + K0
        h, d = a * s, 2.0 * t * s * c * du + s
        inner = 2.0 * du * du * (c - s) + 6.0 * K1 * t
        return h, d, 2.0 * s * c * (t * inner + 2.0 * du)
    raise ValueError(act)


def torch_reference(act, a):
    f = {"sigmoid": torch.sigmoid, "swish": lambda x: x * torch.sigmoid(x),
         "elu": lambda x: torch.where(x >= 0, x, torch.expm1(x)),
         "gelu": lambda x: torch.nn.functional.gelu(x, approximate="tanh")}[act]
    x = torch.tensor(a, dtype=torch.float64, requires_grad=True)
    h = f(x)
    (d,) = torch.autograd.grad(h.sum(), x, create_graph=True)
    (dd,) = torch.autograd.grad(d.sum(), x)
    return h.detach().numpy(), d.detach().numpy(), dd.numpy()


@pytest.mark.parametrize("act", sorted(NEW_IDS))
def test_closed_forms_of_act_prime_and_act_second_equal_double_backward(act):
    """The formulas are a numpy restatement of the device code, so this test pins the mathematics, not the kernels (it would pass
    without them, and cannot see the device code drift from it): the GPU gradient tests, whose act'' term is shown to matter,
    pin what act_fwd_rt / act_dd_rt compute."""
    a = np.concatenate([np.linspace(-88.0, 88.0, 3521), [0.0, -1e-9, 1e-9, -0.03, 0.03, -1e-3, 1e-3]])
    h, d, dd = closed_forms(act, a)
    hr, dr, ddr = torch_reference(act, a)
    assert np.all(np.isfinite(h)) and np.all(np.isfinite(d)) and np.all(np.isfinite(dd))
    np.testing.assert_allclose(h, hr, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(d, dr, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(dd, ddr, rtol=1e-10, atol=1e-13)


@pytest.mark.parametrize("act", sorted(NEW_IDS))
def test_closed_forms_stay_finite_in_float32_for_every_finite_input(act):
    """The same arithmetic in float32, out to the largest finite values (GELU's u' and a u'^2 overflow past |a| ~ 1e8 without
    the clamp of gelu_tail)."""
    big = np.float32(np.finfo(np.float32).max)
    a = np.array([0, 1e-30, 88, 1e3, 1e4, 2e4, 1e7, 2e8, 1e12, 1e19, big], dtype=np.float32)
    a = np.concatenate([a, -a])
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        h, d, dd = closed_forms(act, a)
    assert h.dtype == np.float32 and d.dtype == np.float32 and dd.dtype == np.float32
    assert not np.any(np.isnan(h)) and np.all(np.isfinite(d)) and np.all(np.isfinite(dd)), (h, d, dd)


@pytest.mark.parametrize("act", ["sigmoid", "swish", "elu", "gelu"])
def test_machine_file_keeps_the_new_activations(act, pkg, tmp_path):
    """save_machine stores each layer's activation by name, and load_machine maps the name back to the same id."""
    f = getattr(pkg, act)
    icnf = pkg.ICNF(nvariables=2, naugments=0, nn=pkg.Chain(pkg.Dense(3, 8, f), pkg.Dense(8, 8, pkg.tanh), pkg.Dense(8, 2, f)))
    planar = pkg.ICNF(nvariables=2, naugments=0, nn=pkg.Chain(pkg.PlanarLayer(3, 2, f)))
    for flow, key, want in ((icnf, "dense", [act, "tanh", act]), (planar, "planar", [act])):
        ps, st = pkg.setup(torch.Generator().manual_seed(3), flow)
        path = str(tmp_path / f"{act}-{key}.pt")
        pkg.save_machine(path, pkg.ICNFModel(icnf=flow), (ps, st))
        net = torch.load(path, map_location="cpu", weights_only=True)["icnf"]["net"][key]
        assert (net[2:3] if key == "planar" else [l[2] for l in net]) == want
        model2, _ = pkg.load_machine(path, device="cuda:0")
        assert [l.act_id for l in model2.icnf.nn.layers] == [l.act_id for l in flow.nn.layers]
