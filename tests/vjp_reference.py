"""fp64 reference of the solve as a differentiable function (helper of test_vjp_host.py / test_vjp_gpu.py, not a test).

`integrate` is the Runge-Kutta loop of oracle/cnf_oracle64.py's `loss_and_grad` around its augmented dynamics, with the parameters
and the initial state as torch leaves and the FINAL STATE returned instead of the loss: whatever scalar a test builds on it is
differentiated by torch in float64.  The oracle itself is not edited; its `_act` knows identity / tanh / softplus only, so the
sigmoid / swish / ELU / GELU chains use the plain-torch table below."""
import math

import numpy as np
import torch


def act(a, kind):
    if kind == 0:
        return a
    if kind == 1:
        return torch.tanh(a)
    if kind == 2:
        return torch.nn.functional.softplus(a)
    if kind == 4:
        return torch.sigmoid(a)
    if kind == 5:
        return a * torch.sigmoid(a)
    if kind == 6:
        return torch.where(a >= 0, a, torch.expm1(a))
    if kind == 7:
        return torch.nn.functional.gelu(a, approximate="tanh")
    raise ValueError(kind)


def _layers(spec, pt):
    w_off, b_off, _ = spec.param_offsets()
    out = []
    for l in range(len(spec.acts)):
        fin, fout = spec.widths[l], spec.widths[l + 1]
        out.append((pt[w_off[l]:w_off[l] + fin * fout].reshape(fin, fout).t(), pt[b_off[l]:b_off[l] + fout]))
    return out


def _net(spec, layers, z, t, ys):
    rows = [z]
    if not spec.autonomous:
        rows.append(torch.full((1, z.shape[1]), float(t), dtype=z.dtype))
    if spec.ncond:
        rows.append(ys)
    h = torch.cat(rows, dim=0)
    for (W, b), kind in zip(layers, spec.acts):
        h = act(W @ h + b[:, None], kind)
    return h


def leaf(a, requires_grad=True):
    return torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=requires_grad)


def integrate(o64, spec, p, u0, t0, t1, nsteps=None, alg=1, eps=None, ys=None, tgrid=None):
    """u1 (S, B), a float64 tensor with a graph to `p` and `u0` where those are tensors that require grad (arrays are taken as
    constants).  Steps: `nsteps` equal ones from t0 to t1, or the times of `tgrid`."""
    D, K = spec.D, spec.nprobes
    pt = p if isinstance(p, torch.Tensor) else leaf(p, False)
    u = u0 if isinstance(u0, torch.Tensor) else leaf(u0, False)
    B = u.shape[1]
    layers = _layers(spec, pt)
    e = None if spec.mode == o64.MODE_EXACT else leaf(eps, False)
    yt = None if ys is None else leaf(ys, False)

    def f_aug(u, t):
        z = u[:D]
        if not z.requires_grad:
            z = z.clone().requires_grad_(True)
        zdot = _net(spec, layers, z, t, yt)
        ldot = torch.zeros(B, dtype=torch.float64)
        ndot = torch.zeros(B, dtype=torch.float64)
        if spec.mode == o64.MODE_EXACT:
            for i in range(D):
                seed = torch.zeros_like(zdot)
                seed[i] = 1.0
                (gi,) = torch.autograd.grad(zdot, z, seed, create_graph=True)
                ldot = ldot - gi[i]
            return torch.cat([zdot, ldot[None], torch.zeros(2, B, dtype=torch.float64)], dim=0)
        for k in range(K):
            ek = e[k * D:(k + 1) * D]
            if spec.mode == o64.MODE_HUTCH_VJP:
                (g,) = torch.autograd.grad(zdot, z, ek, create_graph=True)
            else:
                v = torch.zeros_like(zdot, requires_grad=True)
                (jt,) = torch.autograd.grad(zdot, z, v, create_graph=True)
                (g,) = torch.autograd.grad(jt, v, ek, create_graph=True)
            ldot = ldot - (g * ek).sum(0) / K
            if spec.reg_j:
                ndot = ndot + torch.sqrt((g * g).sum(0)) / K
        Edot = torch.sqrt((zdot * zdot).sum(0)) if spec.reg_z else torch.zeros(B, dtype=torch.float64)
        return torch.cat([zdot, ldot[None], Edot[None], ndot[None]], dim=0)

    c, a, b = o64.tableau(alg)
    n_total = nsteps if tgrid is None else len(tgrid) - 1
    dt = (t1 - t0) / n_total if tgrid is None else None
    for n in range(n_total):
        tn = t0 + n * dt if tgrid is None else float(tgrid[n])
        if tgrid is not None:
            dt = float(tgrid[n + 1]) - float(tgrid[n])
        ks = []
        for i in range(len(c)):
            ui = u
            for j, aij in enumerate(a[i]):
                if aij != 0.0:
                    ui = ui + dt * aij * ks[j]
            ks.append(f_aug(ui, tn + c[i] * dt))
        for bi, ki in zip(b, ks):
            u = u + dt * bi * ki
    return u


def pullback(o64, spec, p, u0, u1_bar, t0, t1, nsteps=None, alg=1, eps=None, ys=None, tgrid=None):
    """(grad_p, u0_bar, u1) in float64 numpy: the cotangent `u1_bar` (S, B) pulled back through `integrate`."""
    pt, ut = leaf(p), leaf(u0)
    u1 = integrate(o64, spec, pt, ut, t0, t1, nsteps, alg, eps, ys, tgrid)
    gp, gu = torch.autograd.grad((u1 * leaf(u1_bar, False)).sum(), (pt, ut), allow_unused=True)
    gu = torch.zeros_like(ut) if gu is None else gu
    return gp.numpy(), gu.numpy(), u1.detach().numpy()


def loss_cotangent(spec, u1, lambdas, B):
    """The cotangent under which the pullback is the gradient of the shipped loss mean(-logp + l1 E + l2 n + l3 A) under the
    standard normal: [z1 + l3 z_aug / |z_aug|; 1; l1; l2] / B (rows the flow does not compute carry weight zero there)."""
    D, nv = spec.D, spec.nvars
    u1 = np.asarray(u1, dtype=np.float64)
    bar = np.zeros_like(u1)
    bar[:D] = u1[:D]
    if spec.reg_aug and spec.naug > 0 and lambdas[2] != 0.0:
        za = u1[nv:D]
        nrm = np.sqrt((za * za).sum(0))
        bar[nv:D] += lambdas[2] * za / np.where(nrm > 0, nrm, 1.0)
    bar[D] = 1.0
    bar[D + 1] = lambdas[0]
    bar[D + 2] = lambdas[1]
    return bar / B


def std_normal_logpdf(z):
    return -0.5 * z.shape[0] * math.log(2.0 * math.pi) - 0.5 * (z * z).sum(0)
