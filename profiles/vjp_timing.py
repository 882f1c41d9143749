"""The pullback of the solve against the shipped gradient, alternated in one process (-> profiles/vjp_timing.json):

  * cfg2's shape (FFJORD D = 8, 3 x 64 tanh), B = 65 536, RK4 x 40: cnf_integrate_fixed_vjp on the fused per-wave sweep in its cotangent
    form against cnf_loss_grad_fixed on the same handle - the same MFMAs; the new call reads S x B more floats and holds a few more
    registers per lane;
  * 32 / 3 x 256 tanh, B = 32 768, RK4 x 40: cnf_integrate_fixed_vjp (layer-wise: the cooperative sweeps have no cotangent form)
    against the shipped gradient on its cooperative sweep and forced layer-wise (CNF_GRAD_LAYERED=1 CNF_COOP_GRAD=0) - what leaving those shapes
    layer-wise costs.

python profiles/vjp_timing.py [--resources FILE] [--out FILE]   FILE: a JSON list made from profiles/kernel_resource_table.py's lines for the two fused instances."""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

pkg = entry.load_package()
o64, _ = entry.load_oracle()
lib = pkg._lib
dev = torch.device("cuda:0")


def ptr(t):
    return lib.ptr(t)


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def spread(v):
    return dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), runs=len(v))


def case(nvars, hidden, B, nsteps, reps, also_layered):
    spec = o64.make_spec(nvars=nvars, hidden=hidden)
    p, xs, eps, _ = o64.synth_inputs(spec, B, 20240612)
    widths = spec.widths
    layers = [pkg.Dense(widths[i], widths[i + 1], "tanh" if i + 1 < len(widths) - 1 else "identity") for i in range(len(widths) - 1)]
    icnf = pkg.ICNF(nvariables=nvars, naugments=0, steer_rate=0.0, lambda1=0.0, lambda2=0.0, lambda3=0.0, device=dev,
                    nn=pkg.Chain(*layers), sol_kwargs=dict(alg=pkg.RK4(), adaptive=False, nsteps=nsteps))
    mode = pkg.TrainMode(False)
    h = icnf._handle(mode)
    P = torch.tensor(p, device=dev)
    icnf._bind_params(h, P)
    S = nvars + 3
    x = torch.tensor(xs.T.copy(), device=dev)                                  # column-major: (B, nvars)
    e = torch.tensor(eps.T.copy(), device=dev)
    u0 = torch.cat([x, torch.zeros(B, 3, device=dev)], 1).contiguous()
    bar = torch.randn(B, S, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    grad, gx, sums = torch.empty(P.numel(), device=dev), torch.empty(B, nvars, device=dev), torch.empty(4, device=dev)
    u0_bar, u1 = torch.empty_like(u0), torch.empty_like(u0)
    lam = (C.c_float * 3)(0.0, 0.0, 0.0)
    sp = lib.stream_ptr(dev)

    def shipped():
        lib.check(h.lib.cnf_loss_grad_fixed(h.ptr, lib.ALG_RK4, nsteps, 0.0, 1.0, ptr(x), ptr(e), None, B, lam, ptr(grad), ptr(gx), ptr(sums), sp))

    def vjp():
        lib.check(h.lib.cnf_integrate_fixed_vjp(h.ptr, lib.ALG_RK4, nsteps, 0.0, 1.0, ptr(u0), ptr(e), None, B, ptr(bar), ptr(grad), ptr(u0_bar),
                                                ptr(u1), sp))

    out = dict(shape=f"{nvars} / {len(hidden)} x {hidden[0]} tanh", B=B, alg="RK4", nsteps=nsteps,
               vjp_path=int(h.lib.cnf_vjp_path_for(h.ptr, B, lib.ALG_RK4, 0)), grad_path=int(h.lib.cnf_grad_path_for(h.ptr, B, lib.ALG_RK4, 0)))
    for _ in range(2):                                                          # warm-up: workspaces, code objects, clocks
        shipped()
        vjp()
    torch.cuda.synchronize()
    t_ship, t_vjp, t_lay = [], [], []
    for _ in range(reps):                                                       # alternated: drift hits both alike
        t_ship.append(timed(shipped, 1))
        t_vjp.append(timed(vjp, 1))
    out["cnf_loss_grad_fixed"] = spread(t_ship)
    out["cnf_integrate_fixed_vjp"] = spread(t_vjp)
    out["ratio_of_medians"] = out["cnf_integrate_fixed_vjp"]["median_ms"] / out["cnf_loss_grad_fixed"]["median_ms"]
    if also_layered:
        pkg.set_tuning(grad_layered=1, coop_grad=0)                             # CNF_GRAD_LAYERED=1 CNF_COOP_GRAD=0: no fused, slab or cooperative sweep
        assert int(h.lib.cnf_grad_path_for(h.ptr, B, lib.ALG_RK4, 0)) == 2
        shipped()
        torch.cuda.synchronize()
        for _ in range(reps):
            t_lay.append(timed(shipped, 1))
        pkg.reload_tuning()
        out["cnf_loss_grad_fixed_layered"] = spread(t_lay)
        out["ratio_vjp_to_layered_gradient"] = out["cnf_integrate_fixed_vjp"]["median_ms"] / out["cnf_loss_grad_fixed_layered"]["median_ms"]
    return out


if __name__ == "__main__":
    rec = dict(device=torch.cuda.get_device_name(0), build=pkg._lib.load().cnf_build_info().decode())
    rec["fused_cfg2_shape"] = case(8, [64, 64, 64], 65536, 40, 9, False)
    print(json.dumps(rec["fused_cfg2_shape"]), flush=True)
    rec["layerwise_cooperative_shape"] = case(32, [256, 256, 256], 32768, 40, 3, True)
    print(json.dumps(rec["layerwise_cooperative_shape"]), flush=True)
    if "--resources" in sys.argv:
        rec["kernel_resource_usage"] = json.load(open(sys.argv[sys.argv.index("--resources") + 1]))
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "vjp_timing.json")
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
    print("written", out)
