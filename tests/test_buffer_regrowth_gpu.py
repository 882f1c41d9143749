"""Workspaces that regrow: one handle per kernel family is driven through batch sizes small -> large -> small -> larger, and every
result is compared with that of a fresh handle at the same size.  A handle's device buffers only ever grow (csrc/cnf_devbuf.h), and
several of them are addressed with the column count they were allocated for as a stride (cnf_handle.h: emb.B, adp.B, simt.kbuf_B),
so a capacity that falls out of step with its allocation shows here as a different number - or as a fault.  Every case creates and
destroys its own handles, which also exercises teardown with each combination of used and unused buffers.

Two fresh handles agree bit for bit on every route below (no atomics; the reductions run in a fixed order), so every comparison is
bitwise.  Only ordinary, valid calls are made."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAMES = {0: "identity", 1: "tanh", 2: "softplus"}
SIZES = (40, 520, 40, 1100)          # small -> large -> small -> larger, none a multiple of the 16-sample tile
LAM = (0.01, 0.02, 0.03)

PER_WAVE = dict(nvars=8, hidden=[64, 64, 64], reg_z=True, reg_j=True)                                        # fused per-wave MFMA kernels
SLAB = dict(nvars=7, naug=8, hidden=[64, 64], act=2, reg_z=True, reg_j=True, reg_aug=True)                   # slab-accumulator gradient
COOP = dict(nvars=16, naug=17, hidden=[136, 136], act=2, reg_z=True, reg_j=True, reg_aug=True)               # cooperative kernels
LAYERED = dict(nvars=3, naug=2, ncond=2, hidden=[24, 48, 24], act=2, nprobes=2, reg_aug=True)                # layer-wise gradient
SMALL = dict(nvars=3, naug=2, ncond=2, hidden=[24, 24], act=2, reg_z=True, reg_aug=True)                     # forced onto a generic family


def setsw(pkg, monkeypatch, var, val):
    monkeypatch.setenv(var, str(val))
    pkg.reload_tuning()


def dev(a):
    return None if a is None else torch.tensor(np.asarray(a, dtype=np.float32), device="cuda:0")


def make_icnf(pkg, spec, path=0, **sol):
    layers = [pkg.Dense(spec.widths[i], spec.widths[i + 1], NAMES[spec.acts[i]]) for i in range(len(spec.acts))]
    return pkg.ICNF(nvariables=spec.nvars, naugments=spec.naug, nconditions=spec.ncond, autonomous=spec.autonomous,
                    nn=pkg.Chain(*layers), compute_mode=pkg.HIPVecJacMatrixMode(kernel_path=path), steer_rate=0.0,
                    lambda1=LAM[0] if spec.reg_z else 0.0, lambda2=LAM[1] if spec.reg_j else 0.0,
                    lambda3=LAM[2] if spec.reg_aug else 0.0, nprobes=spec.nprobes, device="cuda:0", sol_kwargs=sol)


def inputs(o64, spec, seed):
    """Parameters and the widest batch; a case takes the leading columns of it."""
    p, xs, eps, ys = o64.synth_inputs(spec, max(SIZES), seed, bias_scale=0.2)
    return (p * 1.5).astype(np.float32), xs, eps, ys


def call_args(spec, p, xs, eps, ys, B):
    args = (dev(xs[:, :B]),) + ((dev(ys[:, :B]),) if spec.ncond else ()) + (dev(p), {})
    return args, dev(eps[:, :B])


def same_bits(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        if isinstance(a, torch.Tensor):
            assert torch.equal(a, b), (what, i, float((a - b).abs().max()))
        else:
            assert a == b, (what, i, a, b)


def drive(make, run):
    """`run` on one long-lived object at every size against `run` on a fresh one."""
    kept = make()
    for B in SIZES:
        same_bits(run(kept, B), run(make(), B), B)


# ---- cnf_inference_fixed ----
@pytest.mark.parametrize("family", ["per_wave", "coop", "layered", "simt"])
def test_inference_fixed_across_regrowth(family, pkg, oracles):
    o64, _ = oracles
    kw, path = {"per_wave": (PER_WAVE, 0), "coop": (COOP, 0), "layered": (SMALL, 3), "simt": (SMALL, 1)}[family]
    spec = o64.make_spec(**kw)
    p, xs, eps, ys = inputs(o64, spec, 3)
    mode = pkg.TrainMode(True)

    def make():
        icnf = make_icnf(pkg, spec, path, alg=pkg.Tsit5(), adaptive=False, nsteps=3)
        fam = icnf.kernel_family(mode)
        assert fam == family or (family == "coop" and fam in ("coop", "coopx", "coopd")), fam
        return icnf

    def run(icnf, B):
        args, e = call_args(spec, p, xs, eps, ys, B)
        logp, regs, u1 = pkg.inference(icnf, mode, *args, eps=e, return_state=True)
        lean = pkg.inference(icnf, mode, *args, eps=e)[0]              # without u_final: the thread-per-sample family's own state slot
        return (logp, *regs, u1, lean)

    drive(make, run)


# ---- cnf_loss_grad_fixed / _grid / _adaptive on each gradient route ----
ROUTES = {"fused": (PER_WAVE, 1), "slab": (SLAB, 1), "coop": (COOP, 3), "layered": (LAYERED, 2)}
ENTRIES = {"fixed": dict(adaptive=False, nsteps=3),
           "grid": dict(adaptive=False, dt=0.3),            # a shorter last step: the grid 0, 0.3, 0.6, 0.9, 1 through cnf_loss_grad_grid
           "adaptive": dict(reltol=1e-4, abstol=1e-4)}


@pytest.mark.parametrize("entry", list(ENTRIES))
@pytest.mark.parametrize("route", list(ROUTES))
def test_loss_grad_across_regrowth(route, entry, pkg, oracles, monkeypatch):
    o64, _ = oracles
    kw, gpath = ROUTES[route]
    if route == "slab":
        setsw(pkg, monkeypatch, "CNF_COOP_GRAD_MID", "0")      # (as the slab kernel's own parity test: no auxiliary cooperative plan)
    spec = o64.make_spec(**kw)
    p, xs, eps, ys = inputs(o64, spec, 5)
    mode = pkg.TrainMode(True)

    def make():
        return make_icnf(pkg, spec, 0, alg=pkg.Tsit5(), **ENTRIES[entry])

    def run(icnf, B):
        args, e = call_args(spec, p, xs, eps, ys, B)
        val, g, gx = pkg.loss_and_gradient(icnf, mode, *args, eps=e, wrt_x=True)
        assert icnf.grad_path(mode, B=B, alg=1, on_grid=entry != "fixed") == gpath
        if entry == "grid":
            assert len(icnf.last_solve_stats["tgrid"]) == 5
        grid = tuple(icnf.last_solve_stats["tgrid"]) if entry == "adaptive" else ()
        return (val, g, gx) + grid

    drive(make, run)


# ---- cnf_solve_vcabm / cnf_solve_tsit5 (one launch, host-driven loop) and cnf_step_embedded (the caller's loop) ----
@pytest.mark.parametrize("controller", ["device", "host", "python"])
@pytest.mark.parametrize("alg", ["VCABM", "Tsit5"])
def test_adaptive_solves_across_regrowth(alg, controller, pkg, oracles, monkeypatch):
    o64, _ = oracles
    if controller == "host":
        setsw(pkg, monkeypatch, "CNF_DEVICE_CONTROLLER", "0")
    spec = o64.make_spec(**PER_WAVE)
    p, xs, eps, ys = inputs(o64, spec, 7)
    mode = pkg.TrainMode(True)

    def make():
        icnf = make_icnf(pkg, spec, 0, alg=getattr(pkg, alg)(), reltol=1e-4, abstol=1e-4)
        if controller == "python":
            icnf.adaptive_policy = "python"     # cnf_step_embedded / cnf_vcabm_* one attempt at a time
        return icnf

    def run(icnf, B):
        args, e = call_args(spec, p, xs, eps, ys, B)
        logp, regs, u1 = pkg.inference(icnf, mode, *args, eps=e, return_state=True)
        st = icnf.last_solve_stats
        if controller != "python":
            assert st["controller"] == controller
        loss = pkg.loss(icnf, mode, *args, eps=e)                       # cnf_loss_adaptive: the same solve from the handle's own state slots
        return (logp, *regs, u1, loss, st["naccept"], st["nreject"]) + tuple(st["dts"])

    drive(make, run)


@pytest.mark.parametrize("family", ["layered", "simt"])
def test_step_embedded_across_regrowth_on_the_generic_families(family, pkg, oracles):
    o64, _ = oracles
    spec = o64.make_spec(**SMALL)
    p, xs, eps, ys = inputs(o64, spec, 9)
    mode = pkg.TrainMode(True)

    def make():
        icnf = make_icnf(pkg, spec, 3 if family == "layered" else 1, alg=pkg.Tsit5(), reltol=1e-4, abstol=1e-4)
        icnf.adaptive_policy = "python"
        return icnf

    def run(icnf, B):
        args, e = call_args(spec, p, xs, eps, ys, B)
        logp, regs, u1 = pkg.inference(icnf, mode, *args, eps=e, return_state=True)
        return (logp, *regs, u1) + tuple(icnf.last_solve_stats["dts"])

    drive(make, run)


# ---- cnf_set_params: a changed layout, host and device pointers in turn ----
def _layouts(spec):
    """The Lux layout, and two others of the same parameters: layers in reverse order behind a gap, and biases first in a longer vector."""
    w0, b0, n0 = spec.param_offsets()
    nl = len(w0)
    size_w = [spec.widths[l] * spec.widths[l + 1] for l in range(nl)]
    size_b = [spec.widths[l + 1] for l in range(nl)]
    w1, b1, o = [0] * nl, [0] * nl, 7
    for l in reversed(range(nl)):
        b1[l], o = o, o + size_b[l]
        w1[l], o = o, o + size_w[l]
    n1 = o + 5
    w2, b2, o = [0] * nl, [0] * nl, 0
    for l in range(nl):
        b2[l], o = o, o + size_b[l] + 3
    for l in range(nl):
        w2[l], o = o, o + size_w[l] + 64
    n2 = o
    return [(w0, b0, n0), (w1, b1, n1), (w2, b2, n2), (w0, b0, n0)], size_w, size_b


def _relayout(p, src, dst, size_w, size_b):
    (ws, bs, _), (wd, bd, nd) = src, dst
    out = np.zeros(nd, dtype=np.float32)
    for l in range(len(ws)):
        out[wd[l]:wd[l] + size_w[l]] = p[ws[l]:ws[l] + size_w[l]]
        out[bd[l]:bd[l] + size_b[l]] = p[bs[l]:bs[l] + size_b[l]]
    return out


@pytest.mark.parametrize("shape", ["per_wave", "slab", "coop", "simt"])
def test_set_params_layouts_and_pointer_kinds(shape, pkg, oracles, monkeypatch):
    o64, _ = oracles
    kw, path = {"per_wave": (PER_WAVE, 0), "slab": (SLAB, 0), "coop": (COOP, 0), "simt": (SMALL, 1)}[shape]
    spec = o64.make_spec(**kw)
    B = 100
    p, xs, eps, ys = inputs(o64, spec, 11)
    L = pkg._lib
    lib = L.load()
    mode = pkg.TrainMode(True)
    layouts, size_w, size_b = _layouts(spec)
    x, e = dev(xs[:, :B].T.copy()), dev(eps[:, :B].T.copy())
    y = dev(ys[:, :B].T.copy()) if spec.ncond else None
    sp = L.stream_ptr(torch.device("cuda:0"))
    lam = (C.c_float * 3)(*LAM)

    def results(icnf, lay, p_lay, on_device):
        h = icnf._handle(mode)
        w_off, b_off, n = lay
        wo, bo = (C.c_size_t * len(w_off))(*w_off), (C.c_size_t * len(b_off))(*b_off)
        src = dev(p_lay) if on_device else torch.tensor(p_lay)
        L.check(lib.cnf_set_params(h.ptr, L.ptr(src), n, wo, bo, int(on_device), sp))
        logp = torch.empty(B, device="cuda:0")
        regs = torch.empty(3, B, device="cuda:0")
        L.check(lib.cnf_inference_fixed(h.ptr, 1, 3, 0.0, 1.0, L.ptr(x), L.ptr(e), L.ptr(y), B, L.ptr(logp), L.ptr(regs), None, sp))
        grad = torch.empty(n, device="cuda:0")
        sums = torch.empty(4, device="cuda:0")
        L.check(lib.cnf_loss_grad_fixed(h.ptr, 1, 3, 0.0, 1.0, L.ptr(x), L.ptr(e), L.ptr(y), B, lam, L.ptr(grad), None, L.ptr(sums), sp))
        torch.cuda.synchronize()
        return logp, regs, sums, grad

    def make():
        return make_icnf(pkg, spec, path, alg=pkg.Tsit5(), adaptive=False, nsteps=3)

    kept = make()
    first = None
    for i, lay in enumerate(layouts):
        p_lay = _relayout(p, layouts[0], lay, size_w, size_b)
        for on_device in ((True, False) if i % 2 == 0 else (False, True)):
            got = results(kept, lay, p_lay, on_device)
            same_bits(got, results(make(), lay, p_lay, on_device), (i, on_device))
            # the same parameters in another layout: the same solve, and the same gradient entries where the layout puts them
            if first is None:
                first = got
            same_bits(got[:3], first[:3], (i, on_device, "layout"))
            assert torch.equal(dev(_relayout(got[3].cpu().numpy(), lay, layouts[0], size_w, size_b)), first[3])
