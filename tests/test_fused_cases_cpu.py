"""Certifies, without a GPU, what ``test_gpu_fused_training.py`` runs the fused network training kernel on
(``_fused_cases.py``): the launch geometry as the launch code has it, the margin-filtered rows (kept share, margin, no ReLU mask
that an fp32 evaluation flips, every row compared), the written-out fp64 reference against autograd through the oracle's
modules, the gradient ladders (exact scaling; which branches of the running-exponent logic each one takes), the refusals of
``mmf_particle_net_train_fused_multi``, and that the derived bound tells a structurally wrong kernel from a rounding one.

The caps are conditions on the INPUTS: a seed that breaks one is replaced, the cap stays.

Smallest fault-to-bound ratio found, over the four networks, on each case family's own launches:

    family       tile / group x 2, x 1/2 / slot     one row dropped      one row dropped
                 (worst layer of dW)                (best layer of dW)   (its compact rows)
    edges        32                                 7.4                  1382
    walk         19                                 32                   1976
    in place     102                                104                  2015
    ascending    396                                103                  2027
    descending   44                                 51                   1989
    zeros        315                                176                  2022

A workgroup's faults move EVERY layer's ``dW`` past ``WIDE`` = 10 bounds.  One dropped row of up to 1025 is the weakest: the
bound of a sum assumes every rounding aligned, so the row shows by ``ROW_WIDE`` = 4 bounds in its best layer only; its own
outputs, which the kernel then never writes, show it by 1 / REL_TOL = 10^4 (``d_states``) and ``ROW_OUT_WIDE`` = 500."""
import ctypes

import pytest
import torch

from oracle import models as om

import _fused_cases as fc

ALL_SHAPES = sorted(set(fc.EDGE_SHAPES) | {(N, M) for N, M, _ in fc.WALK_SHAPES} | {fc.ladder_shape(n) for n in fc.LADDERS})
WIDE, ROW_WIDE, ROW_OUT_WIDE = 10.0, 4.0, 500.0


def test_geometry_is_the_launch_codes():
    assert (fc.TILE_ROWS, fc.GROUP_ROWS, fc.MAX_GRID) == (32, 128, 256)
    assert sorted({N * M for N, M in fc.EDGE_SHAPES}) == [1, 31, 32, 33, 35, 127, 128, 129, 133, 257, 258, 259]
    assert [fc.launch(R, 10 ** 6) for R in (1, 128, 129, 257, 513, 1025)] == [(1, 1), (1, 1), (2, 2), (3, 3), (5, 5), (9, 9)]
    assert fc.launch(129, 1) == (2, 1) and fc.launch(40000, 1000) == (313, 256)
    assert [(N * M, S) for N, M, S in fc.WALK_SHAPES] == [(129, 1), (513, 1), (513, 2), (513, 3), (1025, 4)]
    assert fc.walk(513, 1) == [[0, 1, 2, 3, 4]]
    assert fc.walk(513, 2) == [[0, 2, 4], [1, 3]]
    assert fc.walk(513, 3) == [[0, 3], [1, 4], [2]]
    assert [len(w) for w in fc.walk(1025, 4)] == [3, 2, 2, 2]
    # R = 129: the second group is one live row and three dead tiles
    assert fc.group_rows(1, 129) == slice(128, 129)
    # a trajectory straddles the first tile's end (3 x 11) and the first group's end (3 x 43)
    assert 2 * 11 < 32 < 3 * 11 and 2 * 43 < 128 < 3 * 43
    for name, lad in fc.LADDERS.items():
        ks = [k for k in lad.groups if k is not None]
        assert all(-60 <= k <= 40 for k in ks), name
        assert max((N * M for N, M in ALL_SHAPES)) <= 1300
    up = fc.LADDERS["ascending"].groups
    assert up == (0, 3, 13, 31, 40) and fc.LADDERS["descending"].groups == up[::-1]
    assert all(b - a >= 32 for a, b in zip(fc.LADDERS["steep"].groups, fc.LADDERS["steep"].groups[1:]))
    s = fc.row_scale("specks", 256)
    assert s[5] == 0 and s[133] == 0 and s[37] == 2.0 ** -120 and int((s == 1).sum()) == 253


@pytest.mark.parametrize("task,kind", fc.NETS)
def test_rows_keep_the_masks(task, kind):
    """Every shape of every test: the share kept of the network's candidates (all shapes together: the smallest draw nine)
    is at least ``MIN_KEPT_SHARE``, every row has the margin with its own trajectory's term, an fp32 evaluation flips no mask,
    all ``N M`` rows are there, and the activations are f16 numbers."""
    kept, drawn, low, top = 0.0, 0, 1.0, 0.0
    for N, M in ALL_SHAPES:
        c = fc.case(task, kind, N, M)
        assert c.x.shape == (N * M, fc.DIMS[task]) and c.tb.shape == (N, 64) and c.x.dtype == c.tb.dtype == torch.float32
        t, y = fc.truth(task, kind, N, M), fc.yardstick(task, kind, N, M)
        assert t.pre.shape == (N * M, fc.n_sites(kind), 64) and t.d_states.shape[0] == N * M
        m = float(fc.jc.margin(t.pre, n_sites=fc.n_sites(kind)).min())
        assert m >= fc.MARGIN, (N, M, m)
        assert not bool(((t.pre > 0) != (y.pre > 0)).any()), (N, M)
        kept, drawn = kept + c.kept_share * c.candidates, drawn + c.candidates
        low, top = min(low, m), max(top, max(float(a.abs().max()) for a in t.a))
    print(f"FUSED rows task={task} kind={kind} shapes={len(ALL_SHAPES)} candidates={drawn} kept_share={kept / drawn:.4f} "
          f"margin_min={low:.3e} largest_activation={top:.3e}")
    assert kept / drawn >= fc.MIN_KEPT_SHARE
    assert top < 1000.0   # far inside f16 (relu_sat never clamps)


def _autograd(task, kind, N, M, which=0):
    """The same gradients by autograd through the oracle's own modules (``vector_encoder``, ``resblocks.Linear``) in fp64."""
    spec = om.TASKS[task]
    m = om.DynamicsModel(spec) if kind == "dynamics" else om.MeasurementModel(spec, modalities=("pos", "sensors"))
    m.load_state_dict(fc.state_dict(task, kind))
    m = m.double()
    c = fc.case(task, kind, N, M)
    x = c.x.double().requires_grad_(True)
    tb = c.tb.double().requires_grad_(True)
    g = fc.incoming(task, kind, N, M, None, which).double()
    off = fc.join_state_off(kind)
    join = m.shared_layers[0]
    h = m.state_layers(x) @ join.weight[:, off:off + 64].t() + tb.repeat_interleave(M, dim=0)
    blocks = list(m.shared_layers)[1:-1]   # (the measurement model's nn.ReLU, then) the residual blocks
    for b in blocks:
        h = b(h)
    out = m.shared_layers[-1](h)
    d = fc.DIMS[task]
    loss = (g * out[:, :d] * torch.sigmoid(out[:, d:])).sum() if kind == "dynamics" else (g * out).sum()
    res = [m.state_layers[2].block1, m.state_layers[2].block2, None] + [blk for b in blocks if not isinstance(b, torch.nn.ReLU)
                                                                         for blk in (b.block1, b.block2)]
    leaves = [x, tb, join.weight, m.state_layers[0].weight, m.state_layers[0].bias, m.shared_layers[-1].weight,
              m.shared_layers[-1].bias] + [t for r in res if r is not None for t in (r.weight, r.bias)]
    grads = torch.autograd.grad(loss, leaves)
    want = dict(d_states=grads[0], d_traj_bias=grads[1], dW_in=grads[3], db_in=grads[4], dW_head=grads[5], db_head=grads[6])
    dW, db, it = [], [], iter(grads[7:])
    for r in res:
        if r is None:
            dW.append(grads[2][:, off:off + 64])
            db.append(None)
        else:
            dW.append(next(it))
            db.append(next(it))
    return want, dW, db, out.detach()


@pytest.mark.parametrize("task,kind", fc.NETS)
def test_written_out_reference_is_autograd(task, kind):
    N, M = 3, 43
    want, dW, db, out = _autograd(task, kind, N, M)
    t = fc.truth(task, kind, N, M)
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    errs = [rel(t.out, out)] + [rel(getattr(t, k), v) for k, v in want.items()]
    errs += [rel(t.dW[l], dW[l]) for l in range(len(dW))] + [rel(t.db[l], db[l]) for l in range(len(db)) if db[l] is not None]
    # the join layer has no bias of its own in the kernel: its db is the per-trajectory term's gradient summed
    errs.append(rel(t.db[2], want["d_traj_bias"].sum(0)))
    print(f"FUSED reference task={task} kind={kind} against autograd: worst of {len(errs)} tensors {max(errs):.3e}")
    assert len(t.dW) == 3 + 2 * fc.n_res_of(kind) and max(errs) < 1e-12


@pytest.mark.parametrize("task,kind", fc.NETS)
def test_ladders_scale_exactly_and_take_their_branches(task, kind):
    """A power of two on the incoming gradient is a power of two on every gradient, bit for bit; and each ladder drives the
    running exponent where it is meant to (``eacc_walk``: the kernel's rule restated on the fp64 ``dz``)."""
    c = fc.case(task, kind, 3, 43)
    ps = fc.params(task, kind)
    base = fc.reference(ps, kind, 43, c.x, c.tb, c.g[0], torch.float64)
    for k in (-60, 3, 40):
        s = fc.reference(ps, kind, 43, c.x, c.tb, c.g[0] * 2.0 ** k, torch.float64)
        for a, b in zip([s.d_states, s.dz_first, s.d_raw] + s.dz + s.dW + s.db,
                        [base.d_states, base.dz_first, base.d_raw] + base.dz + base.dW + base.db):
            assert torch.equal(a, b * 2.0 ** k)
        assert all(torch.equal(a, b) for a, b in zip(s.a, base.a))

    def branches(name, n_slots):
        N, M = fc.ladder_shape(name)
        return fc.eacc_walk(fc.truth(task, kind, N, M, name), N * M, n_slots)

    for name in ("ascending", "steep", "up_down_up"):
        L = len(fc.LADDERS[name].groups)
        steps = L - 1 if name != "up_down_up" else 2
        assert all(b["rescales"] == steps for b in branches(name, 1)), name
        assert all(b["rescales"] == 0 for b in branches(name, L)), name        # one group per workgroup: never
    assert all(b["rescales"] == 0 and b["dropped"] >= 128 for b in branches("descending", 1))
    assert all(b["dropped"] < 8 for b in branches("descending", 5))   # (push: a row 2^32 below its own group's largest)
    assert all(b["dropped"] > 0 for b in branches("up_down_up", 1))
    assert all(b["idle"] == 1 and b["rescales"] == 1 and b["not_ok"] >= 3 * 128 for b in branches("zero_groups", 1))
    assert all(b["idle"] == 3 for b in branches("zero_groups", 5))
    assert all(b["not_ok"] == 3 and b["rescales"] <= 1 for b in branches("specks", 1))
    assert all(b["idle"] == 2 and b["not_ok"] == 256 for b in branches("all_zero", 1))
    t = fc.truth(task, kind, *fc.ladder_shape("all_zero"), "all_zero")
    assert not any(bool(w.any()) for w in t.dW + t.db) and not bool(t.d_states.any())


def _family_launches():
    fam = {"edges": [(N, M, fc.launch(N * M, 10 ** 6)[0], None) for N, M in fc.EDGE_SHAPES if N * M > 32],
           "walk": [(N, M, S, None) for N, M, S in fc.WALK_SHAPES],
           "in place": [(27, 19, 2, None)]}
    for name, f in fc.FAMILY.items():
        if name != "all_zero":
            L = len(fc.LADDERS[name].groups)
            fam.setdefault(f, []).extend([fc.ladder_shape(name) + (S, name) for S in (1, L)])
    return fam


@pytest.mark.parametrize("task,kind", fc.NETS)
def test_bound_tells_a_structural_fault_from_rounding(task, kind):
    """Every emulated fault of a workgroup -- the last live tile dropped, one group's contribution scaled by 2 or by 1/2, one
    slot's partial lost -- moves some entry of EVERY layer's ``dW`` past ``WIDE`` times its bound, on every launch of every
    family.  ONE dropped row (the ragged end's) is one of up to 1025 terms of a sum whose bound assumes every rounding aligned:
    it is past ``ROW_WIDE`` times the bound in some layer, and what catches it is the row's own outputs -- ``d_states`` and
    the compact rows the kernel then never writes -- at 1 / REL_TOL and ``ROW_OUT_WIDE`` times their bounds.  An fp32
    evaluation of the same formulas stays inside every bound."""
    for fam, launches in _family_launches().items():
        smallest, smallest_row, smallest_out, inside = float("inf"), float("inf"), float("inf"), 0.0
        for N, M, S, ladder in launches:
            R = N * M
            t, y = fc.truth(task, kind, N, M, ladder), fc.yardstick(task, kind, N, M, ladder)
            bW, bb = fc.weight_bounds(t, y)
            row_best = 0.0
            for l in range(len(bW)):
                inside = max(inside, fc.ratio(y.dW[l], t.dW[l], bW[l]), fc.ratio(y.db[l], t.db[l], bb[l]))
                for name, wrong in fc.faults(t, R, S, l).items():
                    r = fc.ratio(wrong, t.dW[l], bW[l])
                    if name == "last row dropped":
                        row_best = max(row_best, r)
                    else:
                        assert r > WIDE, (fam, N, M, S, ladder, l, name, r)
                        smallest = min(smallest, r)
            assert row_best > ROW_WIDE, (fam, N, M, S, ladder, row_best)
            smallest_row = min(smallest_row, row_best)
            last = fc.top_group_last_row(t, R)
            for want, yard, floor in ((t.dz_first, y.dz_first, True), (t.dz[2], y.dz[2], True), (t.a[-1], y.a[-1], False)):
                b = fc.compact_bound(want, yard, floor)
                inside = max(inside, fc.ratio(yard, want, b[:, None]))
                smallest_out = min(smallest_out, fc.ratio(torch.zeros(64), want[last], b[last]))
            assert float(fc.row_rel(y.d_states, t.d_states).max()) < fc.REL_TOL
        print(f"FUSED discrimination task={task} kind={kind} family={fam}: smallest fault / bound {smallest:.1f} (tile, group, "
              f"slot; every layer), {smallest_row:.1f} (one row; its best layer), {smallest_out:.0f} (one row; its compact rows); "
              f"the fp32 reference / bound {inside:.3f}")
        assert inside < 1.0 and smallest_out > ROW_OUT_WIDE


def test_multi_refuses_what_one_grid_cannot_run():
    """``mmf_particle_net_train_fused_multi`` (the networks of one launch share its grid): ``MMF_EINVAL`` before any launch
    for a dynamics network in the list, differing ``N`` / ``M`` / ``d`` / ``n_slots``, shared ``d_states`` / ``pw`` /
    ``dz_first_h``, and a count of 0 or above ``MMF_LOOP_MAX_MEAS``.  The pointers are never dereferenced."""
    from multimodalfilter_amd import _abi

    lib = _abi.load()
    EINVAL = -1

    def nets(n, **change):
        arr = (_abi.MmfTrainFusedArgs * max(n, 1))()
        for i in range(n):
            a = arr[i]
            a.n_res, a.kind, a.d, a.N, a.M, a.n_slots = 2, 1, 3, 27, 19, 2
            for j, (name, typ) in enumerate(_abi.MmfTrainFusedArgs._fields_):
                if typ is not ctypes.c_int32 and name != "d_states_base":
                    setattr(a, name, 4096 * (1 + j + 64 * i))   # distinct, non-null, never read
        for name, v in change.items():
            setattr(arr[n - 1], name, v)
        return arr

    call = lambda arr, n: lib.mmf_particle_net_train_fused_multi(arr, n, None)
    assert call(nets(2), 0) == EINVAL and call(None, 2) == EINVAL
    assert call(nets(fc.MAX_MEAS + 1), fc.MAX_MEAS + 1) == EINVAL
    for n in (2, 3):
        first = nets(n)[0]
        assert call(nets(n, kind=0, n_res=3, g_next=8, d_raw=16, act=24, g_act=32), n) == EINVAL   # a dynamics network
        for field, v in (("N", 28), ("M", 20), ("d", 2), ("n_slots", 3), ("n_res", 3), ("d_states", first.d_states),
                         ("pw", first.pw), ("dz_first_h", first.dz_first_h), ("d_out", None), ("pb", None)):
            assert call(nets(n, **{field: v}), n) == EINVAL, (n, field)
    # the same lists with N = 0 are accepted as an empty batch: it is the changed field that was refused above
    assert call(nets(2, N=0), 2) == EINVAL
    empty = nets(2)
    empty[0].N = empty[1].N = 0
    assert call(empty, 2) == 0
