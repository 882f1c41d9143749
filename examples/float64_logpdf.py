"""A Float64 flow: train in Float32, evaluate densities in Float64.

The flow of examples/usage.py (softplus 4 => 16 => 16 => 3, one variable + two augmented dimensions) is fitted for a few epochs in
Float32 - training is Float32 only - and its parameters are then handed, converted explicitly, to a twin built with
data_type=torch.float64.  The twin's ICNFDist evaluates logpdf with the exact trace (TestMode) on the double-precision kernel,
fixed-step Tsit5.  Printed: the log-density of a tail point, a log likelihood ratio of two points, how far the Float32 evaluation
of the same numbers is from the Float64 one, and that generate inverts inference to rounding.  One JSON line."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

pkg = entry.load_package()
torch.manual_seed(0)


def flow(data_type):
    return pkg.ICNF(data_type=data_type, nvariables=1, naugments=2, device="cuda:0", steer_rate=0.0,
                    nn=pkg.Chain(pkg.Dense(4, 16, pkg.softplus), pkg.Dense(16, 16, pkg.softplus), pkg.Dense(16, 3)),
                    sol_kwargs=dict(alg=pkg.Tsit5(), adaptive=False, nsteps=64))


# fit in Float32
r = torch.distributions.Beta(2.0, 4.0).sample((1024, 1))
f32 = flow(torch.float32)
model = pkg.ICNFModel(icnf=f32, batchsize=1024, epochs=30, callback=None, init_rng=torch.Generator().manual_seed(1),
                      shuffle_rng=torch.Generator().manual_seed(2))
(ps32, st), _, report = model.fit(r)

# evaluate in Float64: the same parameters, converted explicitly (a Float32 tensor given to a Float64 flow is a TypeError)
f64 = flow(torch.float64)
ps64 = ps32.to(torch.float64)
d64 = pkg.ICNFDist(f64, pkg.TestMode(), ps64, st)
d32 = pkg.ICNFDist(f32, pkg.TestMode(), ps32, st)
pts = torch.tensor([[0.25, 0.999]], dtype=torch.float64, device="cuda:0")       # the mode region and a tail point
lp64 = d64.logpdf(pts)
lp32 = d32.logpdf(pts.to(torch.float32))
assert lp64.dtype == torch.float64

# generate inverts inference: z = T(x), x' = T^-1(z) on the same steps
_, _, u1 = pkg.inference(f64, pkg.TestMode(), pts, ps64, st, return_state=True)
back = pkg.generate(f64, pkg.TestMode(), ps64, st, pts.shape[1], z0=u1[:3].contiguous())

print(json.dumps({
    "fit_final_loss_float32": report["stats"]["final_loss"],
    "logpdf_float64": lp64.tolist(),
    "log_likelihood_ratio_float64": float(lp64[0] - lp64[1]),
    "float32_minus_float64": (lp32.double() - lp64).tolist(),
    "generate_of_inference_minus_x": (back - pts).abs().max().item(),
}))
