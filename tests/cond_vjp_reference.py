"""fp64 reference of the solve of a CONDITIONED flow as a differentiable function of the conditions too (helper of
test_cond_vjp_host.py / test_cond_vjp_gpu.py, not a test).

vjp_reference.integrate turns `ys` into a constant; here it is a torch leaf like `p` and `u0`, so torch differentiates any scalar
built on the final state with respect to it in float64.  The dynamics are vjp_reference's (`_net`, `_layers`, `act`), the
Runge-Kutta loop is the same; test_cond_vjp_host.py checks that both agree on everything they share and that `ys_bar` agrees with
central differences of this solve."""
import torch

from vjp_reference import _layers, _net, act, leaf  # noqa: F401  (act: re-exported for the tests)


def integrate(o64, spec, p, u0, ys, t0, t1, nsteps=None, alg=1, eps=None, tgrid=None):
    """u1 (S, B), a float64 tensor with a graph to `p`, `u0` and `ys` where those are tensors that require grad (arrays are taken
    as constants).  Steps: `nsteps` equal ones from t0 to t1, or the times of `tgrid`."""
    D, K = spec.D, spec.nprobes
    pt = p if isinstance(p, torch.Tensor) else leaf(p, False)
    u = u0 if isinstance(u0, torch.Tensor) else leaf(u0, False)
    yt = ys if isinstance(ys, torch.Tensor) else leaf(ys, False)
    B = u.shape[1]
    layers = _layers(spec, pt)
    e = None if spec.mode == o64.MODE_EXACT else leaf(eps, False)

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


def pullback(o64, spec, p, u0, ys, u1_bar, t0, t1, nsteps=None, alg=1, eps=None, tgrid=None):
    """(grad_p, u0_bar, ys_bar, u1) in float64 numpy: the cotangent `u1_bar` (S, B) pulled back through `integrate`."""
    pt, ut, yt = leaf(p), leaf(u0), leaf(ys)
    u1 = integrate(o64, spec, pt, ut, yt, t0, t1, nsteps, alg, eps, tgrid)
    gp, gu, gy = torch.autograd.grad((u1 * leaf(u1_bar, False)).sum(), (pt, ut, yt), allow_unused=True)
    gu = torch.zeros_like(ut) if gu is None else gu
    gy = torch.zeros_like(yt) if gy is None else gy
    return gp.numpy(), gu.numpy(), gy.numpy(), u1.detach().numpy()
