"""Per-block comparison of a parameter gradient with its reference (helper of test_grad_instances_*.py, not a test).

The suite's gradient bound, max|g - ref| < 5e-5 max|ref| + 1e-6 over the WHOLE flat parameter vector, is blind to a block whose own
entries are far below the largest one: with `synth_inputs` the time column of W_1, its condition columns and b_1 reach down to 1e-4
of the global maximum on the small conditioned shapes, and there the global bound allows an error of half the block.  Here the same
factor is applied to every parameter block on its own scale, with the floor 1e-7 the suite already uses for `grad_x`."""
import numpy as np

REL = 5e-5      # the project's gradient bound (test_parity_gpu.py, test_vjp_gpu.py), per block instead of globally
FLOOR = 1e-7    # the floor of the grad_x assertions of test_parity_gpu.py


def blocks(spec):
    """[(name, slice)] of the flat Lux-layout parameter vector, in storage order: W_1 split by input column group (state, time,
    conditions - a weight is stored input column by input column, `fout` entries each), every further W_l, every b_l."""
    w_off, b_off, n = spec.param_offsets()
    out = []
    H1, o = spec.widths[1], w_off[0]
    groups = [("W1[state]", spec.D), ("W1[time]", 0 if spec.autonomous else 1), ("W1[cond]", spec.ncond)]
    for name, cols in groups:
        if cols:
            out.append((name, slice(o, o + H1 * cols)))
            o += H1 * cols
    assert o == b_off[0], (o, b_off[0])
    out.append(("b1", slice(b_off[0], b_off[0] + H1)))
    for l in range(1, len(spec.acts)):
        fin, fout = spec.widths[l], spec.widths[l + 1]
        out.append((f"W{l + 1}", slice(w_off[l], w_off[l] + fin * fout)))
        out.append((f"b{l + 1}", slice(b_off[l], b_off[l] + fout)))
    assert out[-1][1].stop == n
    return out


def _close(parts, what):
    """parts: [(name, got, want)].  Every part within REL max|want| + FLOOR of its own reference, none of them all zero.
    Returns the largest err / max|want| (to be compared with REL = 5e-5) and prints it with the part it belongs to."""
    worst = (-1.0, 0.0, "", 0.0, 0.0)
    failed = []
    for name, got, want in parts:
        got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
        assert got.shape == want.shape, (what, name, got.shape, want.shape)
        scale = np.abs(want).max()
        assert scale > 0, f"{what}: the reference of {name} is all zero: nothing is compared there"
        err = np.abs(got - want).max()
        bound = REL * scale + FLOOR
        if not err <= bound:                     # (also true for a NaN)
            failed.append((name, err, bound, scale))
        if not err / bound <= worst[0]:
            worst = (err / bound, err / scale, name, err, scale)
    print(f"{what}: worst {worst[2]}: err {worst[3]:.3e} = {worst[1]:.3e} of its max|ref| {worst[4]:.3e} ({worst[0]:.3f} of the bound)")
    assert not failed, (what, [(n, f"err {e:.3e} bound {b:.3e} max|ref| {s:.3e}") for n, e, b, s in failed])
    return worst[1]


def blockwise_close(got, want, spec, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape == (spec.param_offsets()[2],), (what, got.shape, want.shape)
    return _close([(name, got[sl], want[sl]) for name, sl in blocks(spec)], what)


def rowwise_close(got, want, what=""):
    """The same per row of a (rows, B) array: u0_bar[:D], grad_x."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.ndim == 2 and got.shape == want.shape, (what, got.shape, want.shape)
    return _close([(f"row {r}", got[r], want[r]) for r in range(got.shape[0])], what)
