"""The forward-mode Jacobian kernel K5 (the ``kJacobian`` instantiation of ``particle_net_kernel``, ``csrc/particle_net.hip``)
against fp64 on each launch shape, through the C ABI (``mmf_dynamics_jacobian``, ``mmf_dynamics_jacobian_multi``), on the
margin-filtered rows ``_jacobian_cases.py`` builds and ``test_jacobian_cases_cpu.py`` certifies.

The bars come from the reference and the project, not from the kernel.  ``J``: the worst ROW by
``_tol.rel_err(kernel, fp64, dims=2) < max(1e-4, 3 x the fp32 reference's error)``, the rule of ``_guarded_gpu.hold``.
``x'``: ``max|diff| / max|fp64| < 1e-5``, measure and bar of ``test_k2_f16x3_error_against_fp64``.  Every output buffer
carries ``GUARD_ROWS`` sentinel rows past its end, which must come back bit-unchanged.  Each figure is printed before it is
asserted (``pytest -s`` shows them).

Measured on an MI355X, worst over the fourteen row counts of group A (kernel / the fp32 reference, both against fp64):

    task  precision   J, worst row (bar 1e-4)    x' (bar 1e-5)
    door  f32         5.6e-6 / 5.3e-6            6.8e-7 / 7.8e-7
    door  f16x3       9.1e-6 / 5.3e-6            9.6e-7 / 7.8e-7
    push  f32         2.4e-5 / 2.2e-5            3.4e-6 / 3.2e-6
    push  f16x3       2.7e-5 / 2.2e-5            3.4e-6 / 3.2e-6

The tie case (group D): J 9.0e-7 .. 2.0e-6, x' 5.2e-7 .. 7.8e-7.  Group B's comparison ACROSS the two organisations (rows
0 .. 32766 of N = 32767 on 32-column tiles against the same rows of N = 32768 on 64-column tiles) came out bit-identical
for both tasks in both precisions; that is printed, not asserted.  A NaN state (group E) gave a non-finite row in both
precisions and raised the flag in f16x3.
"""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import _jacobian_cases as jc
import _tol
from _guarded_gpu import Out, abi, bits, dev, hold, raw

EINVAL = -1   # include/mmf.h: MMF_EINVAL
_hold = functools.partial(hold, "JACOBIAN")


# ------------------------------------------------------------------------------ models, inputs, launches
def _new_model(task):
    import multimodalfilter_amd as mmf

    return mmf.door_models.DoorDynamicsModel() if task == "door" else mmf.push_models.PushDynamicsModel()


@functools.lru_cache(maxsize=None)
def _model(task, seed, tie=False):
    m = _new_model(task)
    m.load_state_dict(jc.state_dict(task, seed, tie))
    return m.to(dev()).eval()


@functools.lru_cache(maxsize=None)
def _inputs(task, seed):
    """``(x, bias)`` of the whole ``pool(task, seed)`` on the device: a size's inputs are their first ``N`` rows, the same
    bits at every size."""
    p = jc.pool(task, seed)
    with torch.no_grad():
        bias = _model(task, seed).encode_controls(p.u.to(dev()))["bias"]
    return p.x.to(dev()), bias.contiguous()


def _code(precision):
    return abi().PRECISIONS[precision]


def _flag(precision):
    from multimodalfilter_amd import engine

    return engine.range_flag(dev()) if precision != "f32" else None   # as engine.run_jacobian


def _launch(model, precision, x, bias, N):
    """One ``mmf_dynamics_jacobian`` on the first ``N`` rows of ``x`` / ``bias``: the guarded ``(x', J)``."""
    d = x.shape[1]
    xs, jac = Out((N,), (d,)), Out((N,), (d, d))
    code = _code(precision)
    abi().dynamics_jacobian(model._net.blob(code), model._net.n_res, code, x[:N], bias[:N], xs.t, jac.t, _flag(precision), N, d)
    torch.cuda.synchronize()
    return xs, jac


@functools.lru_cache(maxsize=None)
def _run(task, precision, N):
    """The launch of ``case(task, MAIN_SEED, N)``, made once and shared by groups A and B: ``(x', J)`` with their guard rows, on
    the host."""
    xs, jac = _launch(_model(task, jc.MAIN_SEED), precision, *_inputs(task, jc.MAIN_SEED), N)
    return xs.full.cpu(), jac.full.cpu()


def _guards_intact(full, N):
    return bool((full[N:] == jc.SENTINEL).all()) and full.shape[0] == N + jc.GUARD_ROWS


def _check_range():
    from multimodalfilter_amd import engine

    engine.check_range(dev())


def _hold_outputs(group, tag, x_got, J_got, truth, fp32):
    """A's two bars on ``(x', J)`` against the ``Ref``s ``truth`` (fp64) and ``fp32`` (the yardstick)."""
    _hold(group, tag, "J", J_got, truth[1], fp32[1], dims=2)
    assert bool(torch.isfinite(x_got).all()), (group, tag, "x' not finite")
    err, ref = jc.x_err(x_got, truth[0]), jc.x_err(fp32[0], truth[0])
    print(f"JACOBIAN group={group} {tag} what=x' kernel={err:.3e} fp32={ref:.3e} bar={jc.X_BAR:.3e}")
    assert err < jc.X_BAR, (group, tag, "x'", err, ref)


# ------------------------------------------------------------------------------ A: against fp64
@pytest.mark.parametrize("N", jc.NS)
@pytest.mark.parametrize("precision", jc.PRECISIONS)
@pytest.mark.parametrize("task", jc.TASKS)
def test_jacobian_against_fp64(task, precision, N):
    """Group A: every boundary row count of ``launch_ct`` / ``launch_variant`` in both precisions.  N = 16385 is the first
    run of a wave's second 32-column tile, N = 32768 the first of the 64-column organisation (f32: the ``jacobian_outputs``
    epilogue; f16x3: the inline epilogue on a 64-column tile), N = 32777 its last tile half full."""
    x_full, J_full = _run(task, precision, N)
    _check_range()
    assert _guards_intact(x_full, N) and _guards_intact(J_full, N)
    x_got, J_got = x_full[:N], J_full[:N]
    assert not bool((x_got == jc.SENTINEL).any()) and not bool((J_got == jc.SENTINEL).any())
    truth = [t[:N] for t in jc.outputs(task, jc.MAIN_SEED, torch.float64)]
    fp32 = [t[:N] for t in jc.outputs(task, jc.MAIN_SEED, torch.float32)]
    _hold_outputs("A", f"task={task} precision={precision} N={N}", x_got, J_got, truth, fp32)


# ------------------------------------------------------------------------------ B: rows do not depend on their place
@pytest.mark.parametrize("precision", jc.PRECISIONS)
@pytest.mark.parametrize("task", jc.TASKS)
def test_rows_do_not_depend_on_their_place(task, precision):
    """Group B: within one organisation a row carries the same bits wherever it sits -- N = 9 against the first 9 rows of
    65, 16385 and 32767 (32-column tiles), N = 32768 against the first 32768 of 32777 (64-column tiles) --, and two
    identical calls give identical bits.  Across the two organisations the order of the epilogue's operations may differ:
    the difference is printed and each side held to A's bars, no more."""
    short = _run(task, precision, jc.TILE_ROWS + 1)
    for N in (jc.WORKGROUP_ROWS + 1, jc.PASS_ROWS + 1, jc.BIG_N - 1):
        for s, l in zip(short, _run(task, precision, N)):
            assert torch.equal(bits(s[:jc.TILE_ROWS + 1]), bits(l[:jc.TILE_ROWS + 1])), (task, precision, N)
    big, bigger = _run(task, precision, jc.BIG_N), _run(task, precision, jc.POOL_ROWS)
    for s, l in zip(big, bigger):
        assert torch.equal(bits(s[:jc.BIG_N]), bits(l[:jc.BIG_N])), (task, precision)
    for N in (jc.TILE_ROWS + 1, jc.BIG_N):
        again = _launch(_model(task, jc.MAIN_SEED), precision, *_inputs(task, jc.MAIN_SEED), N)
        for s, l in zip(_run(task, precision, N), again):
            assert torch.equal(bits(s), bits(l.full.cpu())), (task, precision, N)
    _check_range()
    # across the organisations
    n = jc.BIG_N - 1
    small = _run(task, precision, n)
    same = all(torch.equal(bits(s[:n]), bits(l[:n])) for s, l in zip(small, big))
    print(f"JACOBIAN group=B task={task} precision={precision} rows=0..{n - 1} 32-column vs 64-column: "
          f"J worst row={_tol.rel_err(big[1][:n], small[1][:n], dims=2):.3e} "
          f"x'={jc.x_err(big[0][:n], small[0][:n]):.3e} bit_identical={same}")
    truth = [t[:n] for t in jc.outputs(task, jc.MAIN_SEED, torch.float64)]
    fp32 = [t[:n] for t in jc.outputs(task, jc.MAIN_SEED, torch.float32)]
    for side, got in (("32-column", small), ("64-column", big)):
        _hold_outputs("B", f"task={task} precision={precision} rows=0..{n - 1} of {side}", got[0][:n], got[1][:n], truth, fp32)


# ------------------------------------------------------------------------------ C: mmf_dynamics_jacobian_multi
@pytest.mark.parametrize("K,N", jc.MULTI_CONFIGS)
@pytest.mark.parametrize("precision", jc.PRECISIONS)
@pytest.mark.parametrize("task", jc.TASKS)
def test_multi_launch_equals_single_launches(task, precision, K, N):
    """Group C: grid ``(grid, K)`` with per-``k`` weights, control terms and offsets into ``states_in`` / ``states_out`` /
    ``jac`` (``pool(task, k)``: states that differ per ``k``): bit-identical to ``K`` single calls, the guard rows behind
    the last ``k`` intact."""
    d = jc.pool(task, 0).x.shape[1]
    code = _code(precision)
    models = [_model(task, k) for k in range(K)]
    ins = [_inputs(task, k) for k in range(K)]
    states = torch.stack([x[:N] for x, _ in ins]).contiguous()
    biases = [b[:N] for _, b in ins]
    blobs = [m._net.blob(code) for m in models]
    assert not torch.equal(states[0], states[1]) and not torch.equal(blobs[0], blobs[1])
    xs, jac = Out((K, N), (d,)), Out((K, N), (d, d))
    packed = (ctypes.c_void_p * K)(*[abi().ptr(b) for b in blobs])
    bias_ptrs = (ctypes.c_void_p * K)(*[abi().ptr(b) for b in biases])
    assert raw("mmf_dynamics_jacobian_multi", packed, models[0]._net.n_res, code, states, bias_ptrs, xs.t, jac.t,
               _flag(precision), K, N, d) == 0
    torch.cuda.synchronize()
    _check_range()
    assert xs.guard_intact() and jac.guard_intact()
    for k in range(K):
        one_x, one_J = _launch(models[k], precision, *ins[k], N)
        assert torch.equal(bits(xs.t[k]), bits(one_x.t)) and torch.equal(bits(jac.t[k]), bits(one_J.t)), (task, precision, K, N, k)
        assert not bool((one_J.t == jc.SENTINEL).any())


# ------------------------------------------------------------------------------ D: the mask rule at a tie
@pytest.mark.parametrize("precision", jc.PRECISIONS)
@pytest.mark.parametrize("task", jc.TASKS)
def test_relu_mask_at_an_exact_zero_is_closed(task, precision):
    """Group D: sixteen first-layer pre-activations are exactly ``0 w + 1 0`` in every row; the tangents must not pass
    there (``pv > 0``, as autograd).  The ``>=`` rule is at least 1e-2 of the row's norm away (CPU test)."""
    t = jc.tie_case(task)
    model = _model(task, jc.MAIN_SEED, True)
    with torch.no_grad():
        bias = model.encode_controls(t.u.to(dev()))["bias"].contiguous()
    xs, jac = _launch(model, precision, t.x.to(dev()), bias, jc.TIE_ROWS)
    _check_range()
    assert xs.guard_intact() and jac.guard_intact()
    truth, fp32 = jc.tie_reference(task, torch.float64), jc.tie_reference(task, torch.float32)
    _hold_outputs("D", f"task={task} precision={precision} N={jc.TIE_ROWS}", xs.t.cpu(), jac.t.cpu(), truth, fp32)


# ------------------------------------------------------------------------------ E: contract edges
@pytest.mark.parametrize("task", jc.TASKS)
def test_zero_rows_and_argument_errors(task):
    """Group E: ``N = 0`` succeeds and writes nothing; a null ``jac`` / ``states_out`` / ``traj_bias``, ``d = 4``, a wrong
    ``n_res`` and an unknown precision are refused with ``MMF_EINVAL`` before any launch, from both entry points."""
    x, bias = _inputs(task, jc.MAIN_SEED)
    model = _model(task, jc.MAIN_SEED)
    d, N, n_res = x.shape[1], 5, model._net.n_res
    blob = model._net.blob(0)
    flag = torch.full((1,), 2, dtype=torch.int32, device=dev())
    xs, jac = Out((2, N), (4,)), Out((2, N), (4, 4))       # (room for K = 2, d = 4: the refused calls' sizes)
    packed, bias_ptrs = (ctypes.c_void_p * 2)(abi().ptr(blob), abi().ptr(blob)), (ctypes.c_void_p * 2)(abi().ptr(bias), abi().ptr(bias))
    x2 = torch.cat([x[:N], x[:N]]).contiguous()

    def single(blob=blob, n_res=n_res, prec=0, x=x, bias=bias, out=xs.t, J=jac.t, N=N, d=d):
        return raw("mmf_dynamics_jacobian", blob, n_res, prec, x, bias, out, J, flag, N, d)

    def multi(packed=packed, n_res=n_res, prec=0, x=x2, bias=bias_ptrs, out=xs.t, J=jac.t, K=2, N=N, d=d):
        return raw("mmf_dynamics_jacobian_multi", packed, n_res, prec, x, bias, out, J, flag, K, N, d)

    for call in (single, multi):
        assert call(N=0) == 0
        for prec in (0, 1):
            assert call(prec=prec, N=0) == 0
        assert call(J=None) == EINVAL
        assert call(out=None) == EINVAL
        assert call(bias=None) == EINVAL
        assert call(x=None) == EINVAL
        assert call(d=4) == EINVAL
        assert call(d=1) == EINVAL
        assert call(n_res=2) == EINVAL
        assert call(n_res=4) == EINVAL
        assert call(prec=2) == EINVAL       # MMF_PREC_BF16: the image encoder's only
        assert call(prec=7) == EINVAL
        assert call(N=-1) == EINVAL
    assert single(blob=None) == EINVAL
    assert multi(packed=None) == EINVAL and multi(K=0) == EINVAL and multi(K=5) == EINVAL    # MMF_LOOP_MAX_MEAS = 4
    null_entry = (ctypes.c_void_p * 2)(abi().ptr(blob), None)
    assert multi(packed=null_entry) == EINVAL
    assert multi(bias=(ctypes.c_void_p * 2)(abi().ptr(bias), None)) == EINVAL
    torch.cuda.synchronize()
    assert xs.untouched() and jac.untouched() and int(flag.item()) == 2


@pytest.mark.parametrize("N", [jc.TILE_ROWS + 1, jc.BIG_N])
def test_range_flag_of_the_jacobian_launch(N):
    """Group E: first-layer weights x 1e5 (as ``test_k2_f16x3_range_flag_reports_saturated_split``) put activations beyond
    the f16 split's range: ``predict_with_jacobian`` raises the flag in f16x3, in both tile organisations, and never in
    f32; the flag is left clear."""
    from multimodalfilter_amd import _abi, engine

    model = _new_model("door")
    model.load_state_dict(jc.state_dict("door", jc.MAIN_SEED))
    with torch.no_grad():
        model.state_layers[0].weight.mul_(1e5)
    model.to(dev()).eval()
    x, u = jc.case("door", jc.MAIN_SEED, N)
    x = x.to(dev())
    ctx = model.encode_controls(u.to(dev()))
    old = engine.DEFAULT_PRECISION
    try:
        engine.set_default_precision("f16x3")
        engine.check_range(dev())  # clear
        mu, A, _ = model.predict_with_jacobian(x, ctx)
        assert mu.shape == (N, 3) and A.shape == (N, 3, 3)
        with pytest.raises(_abi.MmfError, match="f16x3 operand range"):
            engine.check_range(dev())
        engine.check_range(dev())  # the flag was reset
        engine.set_default_precision("f32")
        model.predict_with_jacobian(x, ctx)
        engine.check_range(dev())  # the f32 path never raises it
    finally:
        engine.set_default_precision(old)


@pytest.mark.parametrize("N,r", [(jc.WORKGROUP_ROWS + 1, 19), (jc.POOL_ROWS, jc.BIG_N + 3)])
@pytest.mark.parametrize("precision", jc.PRECISIONS)
@pytest.mark.parametrize("task", jc.TASKS)
def test_a_nan_state_stays_in_its_row(task, precision, N, r):
    """Group E: one NaN state in row ``r``, in the middle of a tile (32-column: row 3 of tile 2; 64-column: row 3 of the
    last, half-empty tile): every other row comes out with the clean call's bits; in f16x3 row ``r`` is non-finite or the
    flag is raised, never a finite row without the flag."""
    from multimodalfilter_amd import engine

    x, bias = _inputs(task, jc.MAIN_SEED)
    clean_x, clean_J = _run(task, precision, N)
    bad = x[:N].clone()
    bad[r, 0] = float("nan")
    xs, jac = _launch(_model(task, jc.MAIN_SEED), precision, bad, bias, N)
    word = engine.range_flag(dev())
    raised = int(word.item()) != 0
    word.zero_()
    assert xs.guard_intact() and jac.guard_intact()
    got_x, got_J = xs.t.cpu(), jac.t.cpu()
    others = torch.arange(N) != r
    assert torch.equal(bits(got_x[others]), bits(clean_x[:N][others])), (task, precision, N)
    assert torch.equal(bits(got_J[others]), bits(clean_J[:N][others])), (task, precision, N)
    finite = bool(torch.isfinite(got_x[r]).all()) and bool(torch.isfinite(got_J[r]).all())
    print(f"JACOBIAN group=E task={task} precision={precision} N={N} NaN row {r}: finite={finite} flag={raised}")
    if precision == "f16x3":
        assert raised or not finite
    else:
        assert not raised and not finite        # x'_0 = fma(dir, s, NaN)
