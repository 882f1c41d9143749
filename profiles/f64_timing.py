"""The double-precision solve (cnf_inference_fixed_f64, csrc/cnf_f64.hip) timed against the only thing a user could do before it
existed - the same solve written in torch.float64 ops on the GPU (matmul forward, autograd VJP for the trace) - and against the
project's own Float32 solve of the same shape (-> profiles/f64_timing.json).

Shapes: cfg2's (FFJORD D = 8, 3 x 64 tanh) and the reference's default architecture at nvariables = 8 (D = 17, 18-72-72-17 softplus,
all three regularisers), RK4 x 40, B = 65 536.  Protocol: every contender runs twice untimed (code objects, allocator, libm tables),
then nine rounds alternate the three in the same process, each call timed with device events; the median of nine is reported with
min / max.  The flop count is the algorithm's (2 (1 + K) sum_l in_l out_l per column and stage evaluation, no padding); the share
of peak is over the f64 MFMA rate MEASURED by profiles/ubench/mfma_f64_peak (its result file, or --peak-tflops).

The default architecture is also timed with its activations replaced by the identity (`f64_kernel_identity_activations`), which
splits the kernel's time into the part the double-precision libm takes and the rest.

python profiles/f64_timing.py [--peak-tflops X] [--out FILE] [--batch B] [--case both|cfg2|default]"""
import argparse
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
dev = torch.device("cuda:0")
NAMES = {0: "identity", 1: "tanh", 2: "softplus"}


def measured_peak(arg):
    if arg:
        return float(arg), "--peak-tflops"
    path = os.path.join(ROOT, "profiles", "ubench", "mfma_f64_peak.result.txt")
    for line in reversed(open(path).read().splitlines()):
        if line.startswith("{"):
            return float(json.loads(line)["measured_peak_tflops"]), os.path.relpath(path, ROOT)
    raise SystemExit("no measured f64 MFMA peak: run profiles/ubench/mfma_f64_peak first")


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def spread(v):
    return dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), runs=len(v))


def torch_solve(spec, layers, x, eps, nsteps, t0=0.0, t1=1.0):
    """The solve as torch.float64 ops: (D, B) tensors, matmul forward, torch.autograd.grad for eps^T J; classic RK4."""
    D, B = spec.D, x.shape[1]
    act = torch.tanh if spec.acts[0] == 1 else torch.nn.functional.softplus
    zeros = torch.zeros(B, device=dev, dtype=torch.float64)

    def f(u, t):
        z = u[:D].detach().requires_grad_(True)
        h = torch.cat([z, torch.full((1, B), t, device=dev, dtype=torch.float64)], 0)
        for i, (W, b) in enumerate(layers):
            h = W @ h + b[:, None]
            if i + 1 < len(layers):
                h = act(h)
        (g,) = torch.autograd.grad(h, z, eps)
        ldot = -(g * eps).sum(0)
        E = torch.linalg.vector_norm(h.detach(), dim=0) if spec.reg_z else zeros
        n = torch.linalg.vector_norm(g, dim=0) if spec.reg_j else zeros
        return torch.cat([h.detach(), ldot[None], E[None], n[None]], 0)

    u = torch.cat([x, torch.zeros(spec.S - spec.nvars, B, device=dev, dtype=torch.float64)], 0)
    dt = (t1 - t0) / nsteps
    for s in range(nsteps):
        t = t0 + s * dt
        k1 = f(u, t)
        k2 = f(u + 0.5 * dt * k1, t + 0.5 * dt)
        k3 = f(u + 0.5 * dt * k2, t + 0.5 * dt)
        k4 = f(u + dt * k3, t + dt)
        u = u + dt / 6.0 * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
    z = u[:D]
    return -0.5 * (z * z).sum(0) - 0.5 * D * np.log(2.0 * np.pi) - u[D]


def case(name, spec, B, nsteps, peak, split_activations=False):
    p, xs, eps, _ = o64.synth_inputs(spec, B, 20240612, bias_scale=0.1)
    reg = bool(spec.reg_z or spec.reg_j or spec.reg_aug)
    mode = pkg.TrainMode(reg)

    def flow(dtype, identity=False):
        nn = pkg.Chain(*[pkg.Dense(spec.widths[i], spec.widths[i + 1], NAMES[0 if identity else spec.acts[i]]) for i in range(len(spec.acts))])
        return pkg.ICNF(data_type=dtype, nvariables=spec.nvars, naugments=spec.naug, nn=nn, steer_rate=0.0, device=dev,
                        lambda1=0.01 if spec.reg_z else 0.0, lambda2=0.01 if spec.reg_j else 0.0, lambda3=0.01 if spec.reg_aug else 0.0,
                        sol_kwargs=dict(alg=pkg.RK4(), adaptive=False, nsteps=nsteps))

    i64, i32 = flow(torch.float64), flow(torch.float32)
    t = lambda a, dt: torch.tensor(a, device=dev, dtype=dt)
    x64, e64, p64 = t(xs, torch.float64), t(eps, torch.float64), t(p, torch.float64)
    x32, e32, p32 = t(xs, torch.float32), t(eps, torch.float32), t(p, torch.float32)
    layers = [(W.to(dev), b.to(dev)) for W, b in o64.unpack_params(spec, p.astype(np.float64))]
    contenders = {
        "f64_kernel": lambda: pkg.inference(i64, mode, x64, p64, {}, eps=e64)[0],
        "torch_float64_ops": lambda: torch_solve(spec, layers, x64, e64, nsteps),
        "f32_solve": lambda: pkg.inference(i32, mode, x32, p32, {}, eps=e32)[0],
    }
    if split_activations:
        # the same launch with every activation replaced by the identity: the same products, LDS traffic and elementwise passes,
        # no libm call - what is left of the kernel's time when the transcendental functions are taken out (a diagnostic, not a
        # contender: it computes another flow)
        lin = flow(torch.float64, identity=True)
        contenders["f64_kernel_identity_activations"] = lambda: pkg.inference(lin, mode, x64, p64, {}, eps=e64)[0]
    out = {}
    for _ in range(2):                                  # pre-roll
        for k, fn in contenders.items():
            out[k] = fn()
    torch.cuda.synchronize()
    times = {k: [] for k in contenders}
    for _ in range(9):                                  # alternate in one process
        for k, fn in contenders.items():
            ms, out[k] = timed(fn)
            times[k].append(ms)
    ref = out["f64_kernel"]
    flops = float(B) * nsteps * 4 * 2.0 * (1 + spec.nprobes) * sum(a * b for a, b in zip(spec.widths[:-1], spec.widths[1:]))
    res = {k: spread(v) for k, v in times.items()}
    med = {k: r["median_ms"] for k, r in res.items()}
    res.update(
        shape=dict(name=name, widths=list(spec.widths), acts=[NAMES[a] for a in spec.acts], B=B, alg="RK4", nsteps=nsteps,
                   regularisers=reg, kernel_path_f32=i32.kernel_family(mode, B)),
        flop=flops,
        f64_kernel_tflops=flops / (med["f64_kernel"] * 1e-3) / 1e12,
        f64_kernel_share_of_measured_mfma_peak=flops / (med["f64_kernel"] * 1e-3) / 1e12 / peak,
        speedup_over_torch_float64_ops=med["torch_float64_ops"] / med["f64_kernel"],
        ratio_to_f32_solve=med["f64_kernel"] / med["f32_solve"],
        max_abs_logp_torch_vs_f64_kernel=float((out["torch_float64_ops"] - ref).abs().max()),
        max_abs_logp_f32_vs_f64_kernel=float((out["f32_solve"].double() - ref).abs().max()),
    )
    print(json.dumps(res["shape"]), {k: round(v, 3) for k, v in med.items()}, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--peak-tflops", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f64_timing.json"))
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--case", choices=("both", "cfg2", "default"), default="both", help="one shape only (for a kernel trace)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("f64_timing.py measures on the GPU; there is nothing to report without one")
    peak, src = measured_peak(a.peak_tflops)
    nv = 8
    D = 2 * nv + 1
    result = dict(
        device=torch.cuda.get_device_name(0), f64_mfma_peak_tflops_measured=peak, peak_source=src,
        protocol="2 untimed runs of each contender, then 9 rounds alternating them in one process; device events; median of 9",
        cases=([case("cfg2: FFJORD 8 / 3 x 64 tanh", o64.make_spec(8, [64, 64, 64], act=1), a.batch, 40, peak)] if a.case != "default" else []) +
              ([case("default architecture at nvariables = 8", o64.make_spec(nv, [4 * (D + 1)] * 2, act=2, naug=nv + 1, reg_z=True, reg_j=True, reg_aug=True),
                     a.batch, 40, peak, split_activations=True)] if a.case != "cfg2" else []))
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
