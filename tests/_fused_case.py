"""One fused network call of the training backward (``mmf_particle_net_train_fused``, C ABI) against the exact-fp32 K6
step kernels (``engine.ParticleNetFunction``): shared by tests/test_gpu_training.py and scripts/debug/fused_check.py."""
import ctypes
import time

import torch

import multimodalfilter_amd as mmf
from multimodalfilter_amd import _abi, engine

U = 64
ROW_OUTPUTS = {"d_states": ("d", torch.float32), "dzf": (U, torch.float16), "scf": (None, torch.float32),
               "dzj": (U, torch.float16), "scj": (None, torch.float32), "hl": (U, torch.float16),
               "d_raw": ("d+1", torch.float32), "act": (U, torch.float32), "g_act": (U, torch.float32)}
FIELDS = {"d_states": "d_states", "dzf": "dz_first_h", "scf": "sc_first", "dzj": "dz_join_h", "scj": "sc_join", "hl": "h_last_h"}


def output_buffers(R, d, NL, S, dev, rows=None):
    """The output buffers of one fused call by the short names used here: the row-indexed ones (``ROW_OUTPUTS``) from
    ``rows(name, shape, dtype)`` (default: ``torch.empty``), the partials ``pw (NL, S, 64, 64)`` / ``pb (NL, S, 64)``
    uninitialised."""
    rows = rows or (lambda name, shape, dtype: torch.empty(shape, dtype=dtype, device=dev))
    width = {"d": d, "d+1": d + 1, U: U}
    bufs = {n: rows(n, (R,) if w is None else (R, width[w]), t) for n, (w, t) in ROW_OUTPUTS.items()}
    bufs["pw"] = torch.empty((NL, S, U, U), dtype=torch.float32, device=dev)
    bufs["pb"] = torch.empty((NL, S, U), dtype=torch.float32, device=dev)
    return bufs


def marshal(blob, n_res, k, d, N, M, S, st, tb, bufs, d_out=None, g_next=None, d_states_base=None):
    """``MmfTrainFusedArgs`` of one call on the tensors given (which the caller keeps alive): ``k`` 0 = dynamics (``g_next``
    and the ``d_raw`` / ``act`` / ``g_act`` buffers), 1 = measurement (``d_out (R,)``)."""
    a = _abi.MmfTrainFusedArgs()
    Pp = lambda t: ctypes.c_void_p(t.data_ptr())
    a.packed_dual, a.n_res, a.kind, a.d, a.N, a.M, a.n_slots = Pp(blob), n_res, k, d, N, M, S
    a.states, a.traj_bias = Pp(st), Pp(tb)
    if k == 0:
        a.g_next, a.d_raw, a.act, a.g_act = Pp(g_next), Pp(bufs["d_raw"]), Pp(bufs["act"]), Pp(bufs["g_act"])
    else:
        a.d_out = Pp(d_out)
    for n, f in FIELDS.items():
        setattr(a, f, Pp(bufs[n]))
    if d_states_base is not None:
        a.d_states_base = Pp(d_states_base)
    a.pw, a.pb = Pp(bufs["pw"]), Pp(bufs["pb"])
    return a


def run_case(task, kind, N, M, seed=0, verbose=True, timing=False, return_rows=False):
    dev = torch.device("cuda:0")
    ns = mmf.door_models if task == "door" else mmf.push_models
    P = task.capitalize()
    torch.manual_seed(seed + N * 100 + M)
    if kind == "dynamics":
        model = ns.DoorDynamicsModelBrent() if task == "door" else getattr(ns, P + "DynamicsModel")()
    else:
        model = getattr(ns, P + "MeasurementModel")(modalities={"pos", "sensors"})
    model.to(dev)
    net = model._net
    d, R = net.d_in, N * M
    NL = 3 + 2 * net.n_res
    g = torch.Generator().manual_seed(5 + seed)
    states = (0.7 * torch.randn((R, d), generator=g)).to(dev).requires_grad_(True)
    tbias = torch.randn((N, U), generator=g).to(dev).requires_grad_(True)
    params = net._sources()
    k = 0 if kind == "dynamics" else 1
    # gradient magnitudes that differ by orders of magnitude between trajectories (particle weights do that)
    row_scale = torch.logspace(0, -4, N).repeat_interleave(M).to(dev)
    out = engine.ParticleNetFunction.apply(net, k, N, M, states, tbias, *params)
    if kind == "dynamics":
        g_next = (torch.randn((R, d), generator=g).to(dev) * row_scale[:, None]).contiguous()
        x_next = out[:, :d] * torch.sigmoid(out[:, d:])
        want = torch.autograd.grad(x_next, [states, tbias, out] + params, g_next)
        d_out_ref = want[2]
        want = want[:2] + want[3:]
    else:
        d_out_ref = (torch.randn((R, 1), generator=g).to(dev) * row_scale[:, None]).contiguous()
        want = torch.autograd.grad(out, [states, tbias] + params, d_out_ref)

    S = min(256, max(1, -(-R // 128)))
    bufs = output_buffers(R, d, NL, S, dev)
    bufs["pw"].zero_(); bufs["pb"].zero_()
    st = states.detach().contiguous()
    tb = tbias.detach().contiguous()
    d_out = None if kind == "dynamics" else d_out_ref.reshape(R).contiguous()
    a = marshal(net.blob(_abi.PREC_F16X3_DUAL), net.n_res, k, d, N, M, S, st, tb, bufs, d_out=d_out,
                g_next=g_next if kind == "dynamics" else None)
    _abi.particle_net_train_fused(a, st)
    torch.cuda.synchronize()
    if timing:
        for _ in range(3):
            _abi.particle_net_train_fused(a, st)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        reps = 20
        for _ in range(reps):
            _abi.particle_net_train_fused(a, st)
        torch.cuda.synchronize()
        print(f"  {task} {kind} {N}x{M}: {(time.perf_counter() - t0) / reps * 1e6:.1f} us per fused call")
        bufs["pw"].zero_(); bufs["pb"].zero_()
        _abi.particle_net_train_fused(a, st)
        torch.cuda.synchronize()

    dW, db = bufs["pw"].sum(1), bufs["pb"].sum(1)
    dz_first = bufs["dzf"].float() * bufs["scf"][:, None]
    dz_join = bufs["dzj"].float() * bufs["scj"][:, None]
    h_last = bufs["hl"].float()
    d_out_used = bufs["d_raw"] if kind == "dynamics" else d_out_ref
    got = {"d_states": bufs["d_states"], "d_traj_bias": dz_join.view(N, M, U).sum(1)}
    grads = [None] * len(params)
    grads[0] = dz_first.t() @ st
    grads[1] = dz_first.sum(0)
    grads[2], grads[3], grads[4], grads[5] = dW[0], db[0], dW[1], db[1]
    gj = torch.zeros_like(params[6])
    gj[:, net.join_state_off:net.join_state_off + U] = dW[2]
    grads[6] = gj
    for i in range(net.n_res):
        for kk in range(2):
            layer = 3 + 2 * i + kk
            grads[7 + 4 * i + 2 * kk] = dW[layer]
            grads[8 + 4 * i + 2 * kk] = db[layer]
    grads[-2] = d_out_used.t() @ h_last
    grads[-1] = d_out_used.sum(0)
    names = ["d_states", "d_traj_bias"] + [f"param{i}{tuple(p.shape)}" for i, p in enumerate(params)]
    gots = [got["d_states"], got["d_traj_bias"]] + grads
    worst = 0.0
    if kind == "dynamics":
        err = float((bufs["d_raw"] - d_out_ref).abs().max()) / max(1e-30, float(d_out_ref.abs().max()))
        worst = max(worst, err)
        if verbose:
            print(f"    d_raw: {err:.2e}")
    for n, a_, b_ in zip(names, gots, want):
        scale = max(1e-30, float(b_.abs().max()))
        err = float((a_.double() - b_.double()).abs().max()) / scale
        bad = not torch.isfinite(a_).all()
        worst = max(worst, err if not bad else float("inf"))
        if verbose:
            print(f"    {n}: {err:.2e}{'  NON-FINITE' if bad else ''}")
    # per-row check of d_states (rows of small trajectories must keep their relative precision)
    rs = want[0].abs().amax(1).clamp_min(1e-30)
    row_err = float(((bufs['d_states'] - want[0]).abs().amax(1) / rs).max())
    print(f"  {task} {kind} {N}x{M}: worst tensor error {worst:.2e}, worst d_states ROW error {row_err:.2e}")
    return (worst, row_err) if return_rows else worst
