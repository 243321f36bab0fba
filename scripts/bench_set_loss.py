"""What training on the particle-set log score costs (profiles/set_loss/README.md): ``mmf_pf_set_nll`` alone, forward and
backward, beside the fp32 torch formulation on the same device; and the optimiser step -- ``train.train_filter_step`` and
``train.GraphedFilterStep`` -- with ``loss="mse"`` and ``loss="nll"``, alternating.

    python scripts/bench_set_loss.py [--reps 5] [--mse-only] [--skip-kernel] [--trace LOSS] [--out FILE]

One JSON document.  ``--mse-only`` touches nothing this feature added (no kernel leg, no ``loss=`` keyword), so the same file
runs on the parent commit.  ``--trace mse|nll``: five eager steps of the reference-sized problem and nothing else -- the
program of a kernel-trace run, whose kernel names and counts are what the ``mse`` step of two commits is compared by.
"""
import os
import statistics
import sys
import time

import torch

import _bench_common as bc

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SCALE = (0.2, 0.2, 0.2)
KERNEL_SHAPES = ((32 * 15, 30), (32 * 20, 4096))            # (rows, particles): the reference's training size, an evaluation-sized set
STEP_SHAPES = (("door", "DoorCrossmodalParticleFilter", 32, 30, 16), ("push", "PushUnimodalParticleFilter", 32, 8192, 16))  # reference, C5


def _events(call, reps, inner):
    for _ in range(20):
        call()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    vals = []
    for _ in range(reps):
        a.record()
        for _ in range(inner):
            call()
        b.record()
        torch.cuda.synchronize()
        vals.append(1e3 * a.elapsed_time(b) / inner)
    return {"median_us": statistics.median(vals), "min": min(vals), "max": max(vals)}


def kernel_case(R, M, reps, dev):
    """The kernel back to back between two events, forward (nll) and backward (the three gradients), and the torch formulation
    of the same two; bytes = 4 (d + 1) per particle read, as many written by the backward."""
    from multimodalfilter_amd import _abi, engine

    d = 3
    g = torch.Generator(device=dev).manual_seed(1)
    X = torch.randn((R, M, d), generator=g, device=dev)
    A = torch.log_softmax(torch.randn((R, M), generator=g, device=dev), dim=1)
    Y = torch.randn((R, d), generator=g, device=dev)
    s = torch.tensor(SCALE, device=dev)
    up = torch.full((R,), 1.0 / R, device=dev)
    E = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    nll, gx, ga, gs = E(R), E(R, M, d), E(R, M), E(R, d)
    inner = 200 if M <= 256 else 50
    out = {"rows": R, "particles": M, "d": d, "bytes_read": 4 * (d + 1) * R * M, "bytes_written_backward": 4 * (d + 1) * R * M}
    out["hip_forward"] = _events(lambda: _abi.pf_set_nll(X, A, Y, s, nll=nll), reps, inner)
    out["hip_backward"] = _events(lambda: _abi.pf_set_nll(X, A, Y, s, up, g_states=gx, g_logw=ga, g_log_scale=gs), reps, inner)
    out["hip_forward"]["bytes_per_s"] = out["bytes_read"] / (1e-6 * out["hip_forward"]["median_us"])
    out["hip_backward"]["bytes_per_s"] = 2 * out["bytes_read"] / (1e-6 * out["hip_backward"]["median_us"])
    Xg, Ag = X.clone().requires_grad_(True), A.clone().requires_grad_(True)
    with torch.no_grad():
        out["torch_forward"] = _events(lambda: engine.particle_set_nll_torch(X, A, Y, s), reps, max(5, inner // 10))

    def torch_both():
        torch.autograd.grad(engine.particle_set_nll_torch(Xg, Ag, Y, s).mean(), (Xg, Ag))

    out["torch_forward_backward"] = _events(torch_both, reps, max(5, inner // 10))
    out["hip_forward_backward_median_us"] = out["hip_forward"]["median_us"] + out["hip_backward"]["median_us"]
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


def step_case(tname, cls, N, M, L, reps, losses, dev):
    """ms per optimiser step (SGD), eager and graphed, the losses alternating inside every repetition."""
    from multimodalfilter_amd import train

    runs = {}
    for name in losses:  # a model and an optimiser of its own for every leg: a captured step owns its gradient buffers
        for mode in ("eager", "graphed"):
            f, batch, cov, d = _problem(tname, cls, N, M, L, dev)
            opt = torch.optim.SGD(f.parameters(), lr=1e-4)
            kw = {} if name == "mse" else {"loss": "nll", "nll_scale": SCALE[:d]}
            if mode == "eager":
                runs[(mode, name)] = lambda f=f, opt=opt, kw=kw: train.train_filter_step(f, batch, opt, initial_covariance=cov, noise=f.noise, **kw)
            else:
                step = train.GraphedFilterStep(f, opt, initial_covariance=cov, noise=f.noise, eager_steps=2, **kw)
                runs[(mode, name)] = lambda step=step: step(batch)
    inner = 10 if M <= 256 else 3
    for run in runs.values():
        for _ in range(4):  # warm-up: allocator, packed-weight caches, the two eager steps and the capture of the graphed step
            run()
    times = {k: [] for k in runs}
    for _ in range(reps):
        for k, run in runs.items():
            times[k].append(1e3 * _timed(lambda: [run() for _ in range(inner)]) / inner)
    out = {"filter": cls, "batch": N, "particles": M, "subsequence": L}
    for (mode, name), v in times.items():
        out.setdefault(mode, {})[name] = {"median_ms_per_step": statistics.median(v), "min": min(v), "max": max(v)}
    return out


def trace(loss, dev):
    from multimodalfilter_amd import train

    tname, cls, N, M, L = STEP_SHAPES[0]
    f, batch, cov, d = _problem(tname, cls, N, M, L, dev)
    opt = torch.optim.SGD(f.parameters(), lr=1e-4)
    kw = {} if loss == "mse" else {"loss": "nll", "nll_scale": SCALE[:d]}
    for _ in range(5):
        train.train_filter_step(f, batch, opt, initial_covariance=cov, noise=f.noise, **kw)
    torch.cuda.synchronize()


def main():
    ap = bc.arg_parser(__doc__)
    ap.set_defaults(reps=5)
    ap.add_argument("--mse-only", action="store_true")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--trace", default=None, choices=("mse", "nll"))
    args = ap.parse_args()
    from multimodalfilter_amd import engine

    dev = torch.device("cuda:0")
    engine.set_training_backend("hip")
    if args.trace:
        trace(args.trace, dev)
        return
    losses = ("mse",) if args.mse_only else ("mse", "nll")
    doc = {}
    if not (args.mse_only or args.skip_kernel):
        doc["kernel"] = [kernel_case(R, M, args.reps, dev) for R, M in KERNEL_SHAPES]
    doc["step"] = [step_case(*shape, args.reps, losses, dev) for shape in STEP_SHAPES]
    bc.write_document(doc, args.out)


if __name__ == "__main__":
    main()
