"""Learned conditions: an encoder in front of a conditioned flow, trained jointly with it.

    python examples/learned_conditions.py

A conditioned flow models p(x | y).  In amortised and simulation-based inference y is not given: an encoder maps raw context (an
observation, a simulator output) to it and is trained together with the flow.  `inference(..., differentiable=True, cond_grad=True)`
makes the solve an autograd node with respect to `ys` as well (the backward is the library's pullback of the solve with the
cotangent of the conditions, cnf_integrate_fixed_vjp_cond), so the encoder is ordinary torch in front of it."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

cnf = entry.load_package()
dev = torch.device("cuda:0")
torch.manual_seed(0)

nvars, ncond, nraw, B = 2, 3, 6, 512
icnf = cnf.ICNF(nvariables=nvars, naugments=0, nconditions=ncond,
                nn=cnf.Chain(cnf.Dense(nvars + 1 + ncond, 32, cnf.tanh), cnf.Dense(32, 32, cnf.tanh), cnf.Dense(32, nvars)),
                steer_rate=0.0, lambda1=0.0, lambda2=0.0, lambda3=0.0, device="cuda:0",
                sol_kwargs=dict(alg=cnf.Tsit5(), adaptive=False, nsteps=8))
encoder = torch.nn.Linear(nraw, ncond).to(dev)

# data whose location depends on the raw context through a map the encoder has to find
raw = torch.randn(B, nraw, device=dev)
xs = (torch.stack([raw[:, 0] + raw[:, 1], raw[:, 2] - raw[:, 3]]) + 0.3 * torch.randn(nvars, B, device=dev))

ps, st = cnf.setup(torch.Generator().manual_seed(1), icnf)
ps = ps.to(dev).requires_grad_()
opt = torch.optim.Adam([ps, *encoder.parameters()], lr=1e-2)
mode = cnf.TrainMode(False)
print("pullback implementation (1 fused, 2 layer-wise):", cnf.vjp_path(icnf, mode, B))
for it in range(30):
    opt.zero_grad()
    ys = encoder(raw).t()                                        # (nconditions, B), with a graph to the encoder
    logp, _ = cnf.inference(icnf, mode, xs, ys, ps, st, differentiable=True, cond_grad=True)
    L = -logp.mean()
    L.backward()                                                 # gradients of the flow AND of the encoder
    opt.step()
    if it % 5 == 0 or it == 29:
        print(f"step {it:2d}  NLL {L.item():.4f}  |grad W_enc| {float(encoder.weight.grad.norm()):.3e}")
