"""CPU: the bookkeeping of the instance census (tests/test_grad_instances_gpu.py) and of the per-block bound (tests/grad_blocks.py) -
every census shape maps to the instance it is meant for, the blocks tile the parameter vector, and the per-block bound sees what
the global one does not."""
import numpy as np
import pytest

import test_grad_instances_gpu as census
import test_vjp_gpu as vjp
from grad_blocks import blocks, blockwise_close


def test_census_shapes_map_to_their_instances_and_reach_all_of_them(oracles):
    o64, _ = oracles
    assert len(census.INSTANCES) == len(set(census.INSTANCES)) == 64
    assert len(census.CENSUS) == 192 and len({f"{census.inst_id(i)}-{f}" for i, f in census.CENSUS}) == 192
    reached = set()
    for inst in census.INSTANCES:
        shapes = census.census_shapes(inst)
        assert [s[0] for s in shapes] == (["small", "large", "D14+t"] if inst[2] == 4 else ["small", "large"])
        for tag, kw, alg, nsteps in shapes:
            for K in (1, 3):
                spec = census.build_spec(o64, kw, nprobes=K)
                assert census.instance_of(spec) == inst, (inst, tag, kw)
            assert spec.naug == (2 if spec.D >= 3 else 0) and spec.reg_z and spec.reg_j and spec.reg_aug == (spec.naug > 0)
            reached.add(census.instance_of(spec))
        # the smallest and the largest: one hidden unit / state row / condition less or more is another instance (or none)
        small, large = shapes[0][1], shapes[1][1]
        HT, L, ZR, CR, ACT = inst
        assert small["hidden"][0] == 16 * (HT - 1) + 1 and large["hidden"][0] == 16 * HT
        assert small["nvars"] + small["naug"] == (1 if ZR == 2 else 9) and not small["autonomous"]
        assert large["nvars"] + large["naug"] + (0 if large["autonomous"] else 1) == (9 if ZR == 2 else 15)
        assert (small["ncond"], large["ncond"]) == ((1, 16) if CR else (0, 0))
    assert reached == set(census.INSTANCES)


def test_the_restated_rule_refuses_what_the_library_refuses(oracles):
    o64, _ = oracles
    ok = dict(nvars=4, hidden=[32, 32], acts=1)
    assert census.instance_of(census.build_spec(o64, ok)) == (2, 2, 2, 0, 1)
    for bad in (dict(ok, nvars=15),                          # 15 state rows + the time column: no room for the bias column
                dict(ok, hidden=[32, 48]), dict(ok, hidden=[80, 80]), dict(ok, hidden=[32]), dict(ok, hidden=[32] * 4),
                dict(ok, ncond=17), dict(ok, acts=7), dict(ok, acts=[1, 2])):
        assert census.instance_of(census.build_spec(o64, bad)) is None, bad
    assert census.instance_of(census.build_spec(o64, dict(ok, nvars=15, autonomous=True))) == (2, 2, 4, 0, 1)


@pytest.mark.parametrize("autonomous", [False, True])
@pytest.mark.parametrize("ncond", [0, 3])
def test_blocks_tile_the_parameter_vector(autonomous, ncond, oracles):
    o64, _ = oracles
    spec = vjp.make_spec(o64, 3, [5, 7], [1, 2], naug=2, ncond=ncond, autonomous=autonomous)
    w_off, b_off, n = spec.param_offsets()
    bl = blocks(spec)
    names = [name for name, _ in bl]
    assert names == (["W1[state]"] + ([] if autonomous else ["W1[time]"]) + (["W1[cond]"] if ncond else [])
                     + ["b1", "W2", "b2", "W3", "b3"])
    cover = np.zeros(n, dtype=int)
    for _, sl in bl:
        assert sl.step is None and 0 <= sl.start < sl.stop <= n
        cover[sl] += 1
    assert np.all(cover == 1)                                 # no gap, no overlap
    # the split of W_1 is by INPUT column: entry (out, in) of a weight lives at w_off + out + fout * in
    d = dict(bl)
    H1, D = 5, 5
    assert d["W1[state]"] == slice(w_off[0], w_off[0] + H1 * D)
    if not autonomous:
        assert d["W1[time]"] == slice(w_off[0] + H1 * D, w_off[0] + H1 * (D + 1))
    if ncond:
        assert d["W1[cond]"].stop == b_off[0] and d["W1[cond]"].stop - d["W1[cond]"].start == H1 * ncond
    assert d["b1"] == slice(b_off[0], b_off[0] + H1) and d["W3"] == slice(w_off[2], w_off[2] + 7 * 5)


def test_blockwise_bound_sees_a_small_block_the_global_bound_does_not(oracles):
    """The smallest conditioned one-tile softplus shape of the census (one hidden unit: every block is a single sum over the batch).
    How far its smallest block lies below the gradient's largest entry depends on the drawn inputs - between 1e-1 and 5e-4 over
    the seeds 0 .. 39 of synth_inputs; seed 29 is one of the small ones.  Scaled by 1.01 or by 1.1 that block passes the suite's
    global bound and fails the per-block one."""
    o64, _ = oracles
    inst = (1, 2, 2, 4, 2)
    tag, kw, alg, nsteps = census.census_shapes(inst)[0]
    assert tag == "small"
    spec = census.build_spec(o64, kw)
    p, xs, eps, ys = o64.synth_inputs(spec, census.B_CENSUS, 29, bias_scale=0.2)
    _, want = o64.loss_and_grad(spec, p, xs, 0.0, 1.0, nsteps, alg, eps, ys, vjp.LAM)
    gmax = np.abs(want).max()
    name, sl = min(blocks(spec), key=lambda b: np.abs(want[b[1]]).max())
    small = np.abs(want[sl]).max()
    print(f"smallest block {name}: {small:.3e} = {small / gmax:.3e} of the global maximum {gmax:.3e}")
    assert 2e-5 < small < 1e-3 * gmax                         # 1 % of it is above the per-block floor and far below the global bound
    blockwise_close(want, want, spec, "the reference itself")
    for what, factor in (("scaled by 1.01", 1.01), ("scaled by 1.1", 1.1)):
        got = want.copy()
        got[sl] *= factor
        vjp.grad_close(got, want, what)                       # the global bound accepts it
        with pytest.raises(AssertionError, match=name.replace("[", r"\[").replace("]", r"\]")):
            blockwise_close(got, want, spec, what)


def test_blockwise_bound_refuses_an_all_zero_reference_block(oracles):
    o64, _ = oracles
    spec = vjp.make_spec(o64, 2, [4, 4], 1)
    want = np.ones(spec.param_offsets()[2])
    want[dict(blocks(spec))["W1[time]"]] = 0.0
    with pytest.raises(AssertionError, match="all zero"):
        blockwise_close(want, want, spec, "zero time column")
