"""A loss of one's own on top of the flow: the solve is a torch.autograd node, the rest is plain torch.

    python examples/custom_loss.py

`inference(..., differentiable=True)` returns logp / E / n / A with gradients to the parameters and the data (the backward is the
library's pullback of the solve, cnf_integrate_fixed_vjp), so what the package's `loss_and_gradient` cannot express - sample
weights, a base distribution other than the standard normal - is ordinary autograd.  `ICNFModel(loss=...)` trains on such a loss."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

cnf = entry.load_package()
dev = torch.device("cuda:0")
torch.manual_seed(0)

nvars = 2
icnf = cnf.ICNF(nvariables=nvars, naugments=0,
                nn=cnf.Chain(cnf.Dense(nvars + 1, 32, cnf.tanh), cnf.Dense(32, 32, cnf.tanh), cnf.Dense(32, nvars)),
                steer_rate=0.0, lambda1=0.0, lambda2=0.0, lambda3=0.0, device="cuda:0",
                sol_kwargs=dict(alg=cnf.Tsit5(), adaptive=False, nsteps=8))
# a base distribution that is not MvNormal(0, I): loss_and_gradient refuses it, autograd through the solve does not care
icnf.basedist = torch.distributions.MultivariateNormal(torch.tensor([0.5, -0.5], device=dev),
                                                       covariance_matrix=torch.diag(torch.tensor([0.5, 2.0], device=dev)))
xs = torch.randn(nvars, 512, device=dev) * 0.5 + 1.0
weights = torch.rand(512, device=dev) + 0.5                     # per-sample weights (importance weights, class balance, ...)


def weighted_nll(icnf, mode, xs, ps, st):
    logp, _ = cnf.inference(icnf, mode, xs, ps, st, differentiable=True)
    return -(weights[:xs.shape[1]] * logp).sum() / weights[:xs.shape[1]].sum()


ps, st = cnf.setup(torch.Generator().manual_seed(1), icnf)
ps = ps.to(dev).requires_grad_()
opt = torch.optim.Adam([ps], lr=5e-3)
mode = cnf.TrainMode(False)
print("pullback implementation (1 fused, 2 layer-wise):", cnf.vjp_path(icnf, mode, xs.shape[1]))
for it in range(20):
    opt.zero_grad()
    L = weighted_nll(icnf, mode, xs, ps, st)
    L.backward()
    opt.step()
    if it % 5 == 0 or it == 19:
        print(f"step {it:2d}  weighted NLL {float(L):.4f}")

# the same loss through the MLJ-style model: fit() differentiates it with torch.autograd.grad
model = cnf.ICNFModel(icnf=icnf, loss=weighted_nll, batchsize=0, epochs=3, eta=5e-3, callback=None)
(ps_fit, _), _, report = model.fit(xs.t().cpu().numpy())
print("ICNFModel(loss=weighted_nll).fit:", report["stats"])
