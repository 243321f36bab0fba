"""What training on the CRPS and the energy score of the particle sets costs (profiles/set_scores/README.md): the forward
(``mmf_pf_scores``), the new backward (``mmf_pf_scores_backward``) and both together, in pairs/s, beside the chunked fp32 torch
formulation (forward + autograd backward) on the same device; and the optimiser step -- ``train.train_filter_step`` and
``train.GraphedFilterStep`` -- with ``loss="mse"``, ``"nll"`` and ``"energy"``, alternating inside each repetition.

    python scripts/bench_set_scores.py [--reps 5] [--skip-kernel] [--skip-step] [--out FILE]

One JSON document.  A pair is one (i, j) of a row's M^2: the forward takes d + 1 sums over it, the backward up to 3 d + 1.
"""
import os
import sys
import time

import torch

import _bench_common as bc

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SCALE = (0.5, 1.0, 2.0)
NLL_SCALE = (0.2, 0.2, 0.2)
KERNEL_SHAPES = ((32 * 15, 30), (32 * 20, 4096))            # (rows, particles): the reference's training size, an evaluation-sized set
STEP_SHAPES = (("door", "DoorCrossmodalParticleFilter", 32, 30, 16), ("push", "PushUnimodalParticleFilter", 32, 8192, 16))  # reference, C5
TORCH_ROWS = 8                                              # rows of one forward + backward of the torch formulation at 4096 particles


def kernel_case(R, M, reps, dev):
    """The kernels back to back between two events and the torch formulation of the same loss, ``sum_rows (sum_k crps_k +
    energy) / R``; the torch leg takes the rows ``TORCH_ROWS`` at a time beyond 256 particles (autograd keeps every (rows, i,
    M, d) chunk for its backward), the kernels take them all at once."""
    from multimodalfilter_amd import _abi, engine

    d = 3
    g = torch.Generator(device=dev).manual_seed(1)
    X = torch.randn((R, M, d), generator=g, device=dev)
    A = torch.log_softmax(torch.randn((R, M), generator=g, device=dev), dim=1)
    Y = torch.randn((R, d), generator=g, device=dev)
    E = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    crps, energy, gx, ga = E(R, d), E(R), E(R, M, d), E(R, M)
    gc, ge = torch.full((R, d), 1.0 / R, device=dev), torch.full((R,), 1.0 / R, device=dev)
    forward = lambda: _abi.pf_scores(X, A, None, Y, crps, energy, None, SCALE)
    backward = lambda: _abi.pf_scores_backward(X, A, None, Y, gc, ge, g_states=gx, g_logw=ga, scale=SCALE)
    crps_only = lambda: _abi.pf_scores_backward(X, A, None, Y, gc, None, g_states=gx, g_logw=ga, scale=SCALE)
    energy_only = lambda: _abi.pf_scores_backward(X, A, None, Y, None, ge, g_states=gx, g_logw=ga, scale=SCALE)
    rows = R if M <= 256 else TORCH_ROWS
    tx, ta = torch.zeros_like(X), torch.zeros_like(A)

    def torch_both():
        for r0 in range(0, R, rows):
            x, a = X[r0:r0 + rows].clone().requires_grad_(True), A[r0:r0 + rows].clone().requires_grad_(True)
            c, e = engine.particle_set_scores_torch(x, a, Y[r0:r0 + rows], SCALE)
            tx[r0:r0 + rows], ta[r0:r0 + rows] = torch.autograd.grad((c.sum() + e.sum()) / R, (x, a))

    inner = 1000 if M <= 256 else 10
    runs = {"hip_forward": (forward, inner), "hip_backward": (backward, inner), "hip_forward_backward": (lambda: (forward(), backward()), inner),
            "hip_backward_crps_only": (crps_only, inner), "hip_backward_energy_only": (energy_only, inner),
            "torch_forward_backward": (torch_both, 20 if M <= 256 else 1)}
    times = bc.time_alternating(runs, reps)
    pairs = R * M * M
    out = {"rows": R, "particles": M, "d": d, "pairs": pairs, "torch_rows_per_call": rows,
           "workspace_bytes": {"forward": _abi.pf_scores_workspace_bytes(R, M, d), "backward": _abi.pf_scores_backward_workspace_bytes(R, M, d)},
           "ms_per_call": {k: bc.stats(v) for k, v in times.items()}}
    out["pairs_per_s"] = {k: pairs / (1e-3 * v["median"]) for k, v in out["ms_per_call"].items()}
    out["torch_over_hip_forward_backward"] = out["ms_per_call"]["torch_forward_backward"]["median"] / out["ms_per_call"]["hip_forward_backward"]["median"]
    backward()
    out["hip_against_torch"] = {"g_states": bc.max_difference(gx, tx), "g_logw": bc.max_difference(ga, ta)}
    return out


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _problem(tname, cls, N, M, L, dev):
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import synthetic

    d = 3 if tname == "door" else 2
    torch.manual_seed(0)
    f = mmf.model_types(tname)[cls]().to(dev).train()
    f.num_particles = M
    f.noise = mmf.NoiseSource(seed=5)
    batch = {k: v.to(dev) for k, v in synthetic.make_trajectories(state_dim=d, T=L - 1, N=N, seed=3).items()}
    return f, batch, torch.eye(d, device=dev) * 0.1, d


def step_case(tname, cls, N, M, L, reps, dev):
    """ms per optimiser step (SGD), eager and graphed, the three losses alternating inside every repetition."""
    from multimodalfilter_amd import train

    runs = {}
    for name in ("mse", "nll", "energy"):  # a model and an optimiser of its own for every leg: a captured step owns its gradient buffers
        for mode in ("eager", "graphed"):
            f, batch, cov, d = _problem(tname, cls, N, M, L, dev)
            opt = torch.optim.SGD(f.parameters(), lr=1e-4)
            kw = {"mse": {}, "nll": {"loss": "nll", "nll_scale": NLL_SCALE[:d]}, "energy": {"loss": "energy", "score_scale": SCALE[:d]}}[name]
            if mode == "eager":
                runs[(mode, name)] = lambda f=f, batch=batch, opt=opt, cov=cov, kw=kw: train.train_filter_step(
                    f, batch, opt, initial_covariance=cov, noise=f.noise, **kw)
            else:
                step = train.GraphedFilterStep(f, opt, initial_covariance=cov, noise=f.noise, eager_steps=2, **kw)
                runs[(mode, name)] = lambda step=step, batch=batch: step(batch)
    inner = 10 if M <= 256 else 3
    for run in runs.values():
        for _ in range(4):  # warm-up: allocator, packed-weight caches, the two eager steps and the capture of the graphed step
            run()
    times = {k: [] for k in runs}
    for _ in range(reps):
        for k, run in runs.items():
            times[k].append(1e3 * _timed(lambda: [run() for _ in range(inner)]) / inner)
    out = {"filter": cls, "batch": N, "particles": M, "subsequence": L, "set_rows": N * (L - 1), "pairs_per_step": N * (L - 1) * M * M}
    for (mode, name), v in times.items():
        out.setdefault(mode, {})[name] = {"ms_per_step": bc.stats(v)}
    return out


def main():
    ap = bc.arg_parser(__doc__)
    ap.set_defaults(reps=5)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    args = ap.parse_args()
    from multimodalfilter_amd import engine

    dev = torch.device("cuda:0")
    engine.set_training_backend("hip")
    doc = {"device": torch.cuda.get_device_name(dev)}
    if not args.skip_kernel:
        doc["kernel"] = [kernel_case(R, M, args.reps, dev) for R, M in KERNEL_SHAPES]
    if not args.skip_step:
        doc["step"] = [step_case(*shape, args.reps, dev) for shape in STEP_SHAPES]
    bc.write_document(doc, args.out)


if __name__ == "__main__":
    main()
