"""GPU: every instance of the fused reverse sweep, in each of its three forms, against float64 autograd - PER PARAMETER BLOCK.

The sweep (csrc/cnf_grad2.hip, host side csrc/cnf_grad.hip) is 64 separately compiled shape instances - HT in {1, 2, 3, 4} hidden
tiles x L in {2, 3} hidden layers x ZR in {2, 4} state k-steps x CR in {0, 4} condition k-steps x {tanh, softplus} - each built as
the one-probe gradient, the several-probe gradient (cnf_grad2_probes.hip) and the cotangent form (cnf_grad2_cot.hip): 192 kernels
that differ in more than their loop bounds (KEEP_D, the HT == 4 tanh branch, GT_SLOT, the spilling widest instances).

1. the census: one case per (instance, form) on the smallest and the largest configuration that resolve to the instance (for ZR = 4
   also D = 14 non-autonomous: time in input column 14 next to the bias column 15), B = 37 = two full sample tiles and a ragged one;
2. a second trip of the sweep's tile loop (`tile += gridDim.x * 4`: B > 64 x the number of compute units), cotangent and
   several-probe forms - per-tile state is re-initialised inside that loop and the u0_bar store sits in its tail;
3. the layer-wise pullback across the 64-column chunks of its weight-cotangent products (B = 150: 64 + 64 + 22).

Bounds: tests/grad_blocks.py - 5e-5 max|ref| + 1e-7 per parameter block and per row of u0_bar / grad_x (the project's gradient
factor on the block's own scale); loss and u1 1e-4 absolute as everywhere.  A float32 run of the reference itself differs from
float64 by at most 5.3e-6 of a block's own maximum on the census shapes (CPU, one probe).

Measured on the MI355X, worst err / max|ref| over all blocks of all census shapes of a form (to be compared with 5e-5):
    one probe      4.7e-6  (HT1-L3-ZR2-CR0-tanh);   at most 0.06 of a block's bound, floor included
    three probes   2.1e-6  (HT1-L3-ZR4-CR4-tanh);   at most 0.04 of a block's bound
    cotangent      2.2e-5  (HT1-L3-ZR4-CR4-tanh small, W_2: ONE hidden unit, so the block is a single sum - of O(1) terms under a
                   Gaussian cotangent - that cancels to 4e-2; err 8.6e-7, 0.41 of its bound); the other one-unit shapes up to 8.1e-6
                   (0.16), every shape with more than one hidden unit below 3.3e-6 (0.07)
    rows of grad_x / u0_bar: at most 1.9e-6 of the row's maximum (0.04 of the bound)
    second trip: cotangent 2.4e-6, two probes 2.0e-7;  layer-wise pullback at B = 150: 1.2e-6
No instance exceeds the bound; the all-zero-block check never fired.
"""
import math

import numpy as np
import pytest
import torch

import test_vjp_gpu as vjp
import vjp_reference as ref
from grad_blocks import blockwise_close, rowwise_close

pytestmark = pytest.mark.gpu

TOL_SOLVE = 1e-4
ACT_NAMES = {1: "tanh", 2: "softplus"}
FORMS = ("one", "k3", "cot")      # one probe; K = 3 probes; the cotangent form (the pullback of the solve)
B_CENSUS = 37

# (HT, L, ZR, CR, ACT): the product of the five axes.  Mirrors GRAD_SHAPES / kGrad in csrc/cnf_grad.hip (and kGrad2 in cnf_grad2.hip).
INSTANCES = [(HT, L, ZR, CR, ACT) for ACT in (1, 2) for CR in (0, 4) for HT in (1, 2, 3, 4) for L in (2, 3) for ZR in (2, 4)]


def inst_id(inst):
    HT, L, ZR, CR, ACT = inst
    return f"HT{HT}-L{L}-ZR{ZR}-CR{CR}-{ACT_NAMES[ACT]}"


def instance_of(spec):
    """grad_find's rule (csrc/cnf_grad.hip) restated from the spec alone: the instance that serves it, or None."""
    hidden, acts = list(spec.widths[1:-1]), list(spec.acts)
    L, H, D = len(hidden), spec.widths[1], spec.D
    if L not in (2, 3) or any(h != H for h in hidden) or any(a != acts[0] for a in acts[:-1]) or acts[-1] != 0:
        return None
    if acts[0] not in ACT_NAMES or spec.ncond > 16 or H > 64:
        return None
    if D + (0 if spec.autonomous else 1) > 15:      # one 16-column input tile whose last column is the bias column
        return None
    return ((H + 15) // 16, L, 2 if D <= 8 else 4, 4 if spec.ncond > 0 else 0, acts[0])


def census_shapes(inst):
    """[(tag, make_spec keywords, alg, nsteps)]: the smallest and the largest configuration of the instance (+ D = 14 with a time
    column for ZR = 4).  naug = 2 wherever D >= 3: the augmented rows straddle the instance's row groups; every regulariser on."""
    HT, L, ZR, CR, ACT = inst

    def kw(H, D, C, autonomous):
        naug = 2 if D >= 3 else 0
        return dict(nvars=D - naug, naug=naug, ncond=C, hidden=[H] * L, acts=ACT, autonomous=autonomous,
                    reg_z=True, reg_j=True, reg_aug=naug > 0)

    small = kw(16 * (HT - 1) + 1, 1 if ZR == 2 else 9, 1 if CR else 0, False)
    large = kw(16 * HT, 8 if ZR == 2 else 15, 16 if CR else 0, ZR == 4)
    out = [("small", small, 0, 2), ("large", large, 1, 2)]
    if ZR == 4:
        out.append(("D14+t", kw(16 * HT, 14, 16 if CR else 0, False), 1, 2))
    return out


def build_spec(o64, kw, nprobes=1):
    kw = dict(kw)
    return vjp.make_spec(o64, kw.pop("nvars"), kw.pop("hidden"), kw.pop("acts"), nprobes=nprobes, **kw)


def check_loss_gradient(pkg, o64, spec, alg, nsteps, B, seed, what):
    """loss_and_gradient (one or several probes) against o64.loss_and_grad; returns the worst block ratio."""
    p, xs, eps, ys = o64.synth_inputs(spec, B, seed, bias_scale=0.2)
    icnf = vjp.make_icnf(pkg, spec, alg, nsteps)
    mode = vjp.mode_of(pkg, spec)
    assert icnf.grad_path(mode, B=B, alg=alg) == 1, what
    args = (vjp.dev(xs),) + ((vjp.dev(ys),) if spec.ncond else ()) + (vjp.dev(p), {})
    val, g, gx = pkg.loss_and_gradient(icnf, mode, *args, eps=vjp.dev(eps), wrt_x=True)
    g, gx = g.cpu().numpy(), gx.cpu().numpy()
    Lr, gr, gxr = o64.loss_and_grad(spec, p, xs, 0.0, 1.0, nsteps, alg, eps, ys, vjp.LAM, wrt_x=True)
    print(f"{what}: loss err {abs(float(val) - Lr):.3e}")
    assert abs(float(val) - Lr) < TOL_SOLVE, what
    ratio = blockwise_close(g, gr, spec, what + " grad")
    rowwise_close(gx, gxr, what + " grad_x")
    return ratio, gx, gxr


def check_cotangent(pkg, o64, spec, alg, nsteps, B, seed, what, path=1):
    """integrate_vjp against vjp_reference.pullback; returns the worst block ratio."""
    p, u0, eps, ys, bar = vjp.inputs(o64, spec, B, seed)
    icnf = vjp.make_icnf(pkg, spec, alg, nsteps)
    assert pkg.vjp_path(icnf, vjp.mode_of(pkg, spec), B, alg) == path, what
    g, u0_bar, u1 = vjp.run_vjp(pkg, icnf, spec, p, u0, eps, ys, bar)
    gr, ur, u1r = ref.pullback(o64, spec, p, u0, bar, 0.0, 1.0, nsteps, alg, eps, ys)
    err = np.abs(u1 - u1r).max()
    print(f"{what}: u1 err {err:.3e}")
    assert err < TOL_SOLVE, what
    ratio = blockwise_close(g, gr, spec, what + " grad")
    D = spec.D
    rowwise_close(u0_bar[:D], ur[:D], what + " u0_bar")
    assert np.array_equal(u0_bar[D:], bar[D:]), what      # the dlogp / E / n rows feed nothing: passed through bit for bit
    return ratio, u0_bar, ur


# ---- 1. the census ----
CENSUS = [(inst, form) for inst in INSTANCES for form in FORMS]


@pytest.mark.parametrize("case", range(len(CENSUS)), ids=[f"{inst_id(i)}-{f}" for i, f in CENSUS])
def test_every_instance_against_fp64_per_block(case, pkg, oracles):
    inst, form = CENSUS[case]
    o64, _ = oracles
    worst = 0.0
    for k, (tag, kw, alg, nsteps) in enumerate(census_shapes(inst)):
        spec = build_spec(o64, kw, nprobes=3 if form == "k3" else 1)
        assert instance_of(spec) == inst, (tag, kw)       # from the spec alone, before the library is asked
        what, seed = f"{inst_id(inst)}-{form} {tag}", 1000 + 10 * case + k
        check = check_cotangent if form == "cot" else check_loss_gradient
        worst = max(worst, check(pkg, o64, spec, alg, nsteps, B_CENSUS, seed, what)[0])
    print(f"CENSUS {form} {inst_id(inst)} worst block ratio {worst:.3e}")


# ---- 2. a second trip of the tile loop ----
SECOND_TRIP = {
    "cfg2": dict(nvars=8, hidden=[64, 64, 64], acts=1, reg_z=True, reg_j=True),
    # ZR = 4, CR = 4, softplus, two layers, a padded hidden width: shares as little as possible with cfg2's instance
    "d14-c16-softplus": dict(nvars=10, naug=4, ncond=16, hidden=[49, 49], acts=2, reg_z=True, reg_j=True, reg_aug=True),
}


@pytest.mark.parametrize("form", ["cot", "k2"])
@pytest.mark.parametrize("name", sorted(SECOND_TRIP))
def test_second_trip_of_the_tile_loop(name, form, pkg, oracles):
    """A wave of the sweep takes tiles `tile += gridDim.x * 4`; with one workgroup per compute unit the second trip starts at
    B > 64 x (number of CUs).  Here most waves do one tile, six do a second one and the last tile is ragged.  The columns of the
    second-trip tiles are also compared on their own: a fault there cannot hide behind the 64 x CUs good columns before them."""
    o64, _ = oracles
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = 64 * cus + 16 * 5 + 7
    assert math.ceil(B / 16) > 4 * cus
    spec = build_spec(o64, SECOND_TRIP[name], nprobes=2 if form == "k2" else 1)
    check = check_cotangent if form == "cot" else check_loss_gradient
    ratio, cols, cols_ref = check(pkg, o64, spec, 1, 1, B, 31, f"second trip {name} {form}")
    rows = spec.D if form == "cot" else spec.nvars
    rowwise_close(cols[:rows, 64 * cus:], cols_ref[:rows, 64 * cus:], f"second trip {name} {form}: columns of the second-trip tiles")
    print(f"SECOND_TRIP {form} {name} worst block ratio {ratio:.3e}")


# ---- 3. the layer-wise pullback across the chunks of its weight-cotangent products ----
@pytest.mark.parametrize("name", ["GELU / sigmoid chain", "K = 4 probes"])
def test_layerwise_pullback_across_weight_cotangent_chunks(name, pkg, oracles):
    """lg_wgrad_chunks (csrc/cnf_lgemm.hip) cuts the weight-cotangent products at multiples of 64 columns: B = 150 is three chunks,
    the last one ragged with 22 columns (the largest B of test_vjp_gpu.py's LAYERED is 30: one chunk)."""
    o64, _ = oracles
    kw, alg, nsteps, _ = vjp.LAYERED[name]
    kw = dict(kw)
    spec = vjp.make_spec(o64, kw.pop("nvars"), kw.pop("hidden"), kw.pop("acts", 1), **kw)
    ratio = check_cotangent(pkg, o64, spec, alg, nsteps, 150, 3, f"layer-wise {name}", path=2)[0]
    print(f"LAYERED {name} worst block ratio {ratio:.3e}")
