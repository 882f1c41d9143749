"""What the cotangent of the conditions costs: the pullback of the solve of a conditioned flow through its three calls, alternated in
one process (-> profiles/cond_vjp_timing.json):

  * cnf_integrate_fixed_vjp                       the entry as it was,
  * cnf_integrate_fixed_vjp_cond, ys_bar = NULL   the same kernels through the new entry,
  * cnf_integrate_fixed_vjp_cond with ys_bar      the kernel of cnf_grad2_coty.hip (path 1) / one more accumulation per stage and one
                                                  product per call (path 2),

for 8 variables / 8 conditions / 3 x 64 tanh (fused per-wave sweep) and 8 / 8 / 3 x 128 tanh (layer-wise), B = 65 536, RK4 x 40: a
pre-roll of two rounds, then 9 samples of each call, round-robin, so drift hits the three alike.

python profiles/cond_vjp_timing.py [--commit HASH] [--parent HASH] [--resources FILE] [--out FILE]
FILE of --resources: a JSON list of the new instances' registers next to their parents' (from profiles/kernel_resource_table.py)."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

pkg = entry.load_package()
o64, _ = entry.load_oracle()
lib = pkg._lib
dev = torch.device("cuda:0")
ptr = lib.ptr


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def spread(v):
    return dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), runs=len(v))


def case(nvars, ncond, hidden, B, nsteps, reps):
    spec = o64.make_spec(nvars=nvars, hidden=hidden, ncond=ncond)
    p, xs, eps, ys = o64.synth_inputs(spec, B, 20240612)
    widths = spec.widths
    layers = [pkg.Dense(widths[i], widths[i + 1], "tanh" if i + 1 < len(widths) - 1 else "identity") for i in range(len(widths) - 1)]
    icnf = pkg.ICNF(nvariables=nvars, naugments=0, nconditions=ncond, steer_rate=0.0, lambda1=0.0, lambda2=0.0, lambda3=0.0, device=dev,
                    nn=pkg.Chain(*layers), sol_kwargs=dict(alg=pkg.RK4(), adaptive=False, nsteps=nsteps))
    h = icnf._handle(pkg.TrainMode(False))
    P = torch.tensor(p, device=dev)
    icnf._bind_params(h, P)
    S = nvars + 3
    e = torch.tensor(eps.T.copy(), device=dev)                                  # column-major: (B, D)
    y = torch.tensor(ys.T.copy(), device=dev)
    u0 = torch.cat([torch.tensor(xs.T.copy(), device=dev), torch.zeros(B, 3, device=dev)], 1).contiguous()
    bar = torch.randn(B, S, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    grad, u0_bar, u1, ys_bar = torch.empty(P.numel(), device=dev), torch.empty_like(u0), torch.empty_like(u0), torch.empty_like(y)
    sp = lib.stream_ptr(dev)
    head = (h.ptr, lib.ALG_RK4, nsteps, 0.0, 1.0, ptr(u0), ptr(e), ptr(y), B, ptr(bar), ptr(grad), ptr(u0_bar))
    calls = {
        "cnf_integrate_fixed_vjp": lambda: lib.check(h.lib.cnf_integrate_fixed_vjp(*head, ptr(u1), sp)),
        "cnf_integrate_fixed_vjp_cond(ys_bar=NULL)": lambda: lib.check(h.lib.cnf_integrate_fixed_vjp_cond(*head, None, ptr(u1), sp)),
        "cnf_integrate_fixed_vjp_cond(ys_bar)": lambda: lib.check(h.lib.cnf_integrate_fixed_vjp_cond(*head, ptr(ys_bar), ptr(u1), sp)),
    }
    out = dict(shape=f"{nvars} / {ncond} cond / {len(hidden)} x {hidden[0]} tanh", B=B, alg="RK4", nsteps=nsteps,
               vjp_path=int(h.lib.cnf_vjp_path_for(h.ptr, B, lib.ALG_RK4, 0)))
    for _ in range(2):                                                          # pre-roll: workspaces, code objects, clocks
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in calls}
    for _ in range(reps):                                                       # alternated: drift hits all three alike
        for k, fn in calls.items():
            t[k].append(timed(fn))
    for k in calls:
        out[k] = spread(t[k])
    base = out["cnf_integrate_fixed_vjp"]["median_ms"]
    out["null_over_old"] = out["cnf_integrate_fixed_vjp_cond(ys_bar=NULL)"]["median_ms"] / base
    out["ys_bar_over_old"] = out["cnf_integrate_fixed_vjp_cond(ys_bar)"]["median_ms"] / base
    return out


def arg(name):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else None


if __name__ == "__main__":
    rec = dict(device=torch.cuda.get_device_name(0), build=pkg._lib.load().cnf_build_info().decode(), commit=arg("--commit"), parent=arg("--parent"))
    rec["fused_8_8_3x64"] = case(8, 8, [64, 64, 64], 65536, 40, 9)
    print(json.dumps(rec["fused_8_8_3x64"]), flush=True)
    rec["layerwise_8_8_3x128"] = case(8, 8, [128, 128, 128], 65536, 40, 9)
    print(json.dumps(rec["layerwise_8_8_3x128"]), flush=True)
    if arg("--resources"):
        rec["kernel_resource_usage"] = json.load(open(arg("--resources")))
    out = arg("--out") or os.path.join(ROOT, "profiles", "cond_vjp_timing.json")
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
    print("written", out)
