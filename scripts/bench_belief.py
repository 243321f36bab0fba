"""What the belief record costs (profiles/belief/README.md): ``forward_loop`` with ``record_belief`` off and on, alternating,
for the door crossmodal particle filter and the door crossmodal EKF; K1 alone with and without its three record outputs;
and the only way to the same quantities without the record -- ``forward`` step by step plus torch reductions of the
particle set.

    python scripts/bench_belief.py [--reps 3] [--steps 64] [--off-only] [--out FILE]

One JSON document.  ``--off-only`` touches nothing this feature added, so the same file runs on the parent commit.
"""
import os
import statistics
import sys
import time

import torch

import _bench_common as bc

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _legs(run, reps, off_only, T):
    """us per step: ``run(record)`` timed ``reps`` times per setting, the settings alternating; median and spread."""
    settings = [False] if off_only else [False, True]
    for rec in settings:
        run(rec)  # warm-up: allocator, packed-weight caches
    times = {rec: [] for rec in settings}
    for _ in range(reps):
        for rec in settings:
            times[rec].append(1e6 * _timed(lambda: run(rec)) / T)
    return {("on" if rec else "off"): {"median_us_per_step": statistics.median(v), "min": min(v), "max": max(v)}
            for rec, v in times.items()}


def pf_case(N, M, T, reps, off_only, dev):
    import bench
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import _abi, engine, synthetic

    d = 3
    torch.manual_seed(0)
    f = mmf.door_models.DoorCrossmodalParticleFilter().to(dev).eval()
    synthetic.stabilise_dynamics(f)
    traj = bench.to_device(synthetic.make_trajectories(state_dim=d, T=T, N=N, seed=5), dev)
    f.num_particles = M
    f.noise = mmf.CounterNoise(7)
    f.reserve(steps=T, batch=N, particles=M)
    obs = {k: traj[k][1:] for k in ("image", "gripper_pos", "gripper_sensors")}
    ctrl = traj["controls"][1:]
    steps = ctrl.shape[0]
    cov0 = (torch.eye(d, device=dev) * 0.1)[None].expand(N, d, d)

    def run(record):
        if record:
            f.record_belief = True
        f.initialize_beliefs(mean=traj["states"][0], covariance=cov0)
        f.forward_loop(observations=obs, controls=ctrl)
        if record:
            f.record_belief = False

    out = {"filter": "DoorCrossmodalParticleFilter", "batch": N, "particles": M, "steps": steps,
           "persistent_eligible": bool(engine.PF_PERSISTENT and _abi.pf_persistent_plan(N, M, 2) > 0),
           "forward_loop": _legs(run, reps, off_only, steps)}
    if not off_only:
        def stepwise_torch():
            f.initialize_beliefs(mean=traj["states"][0], covariance=cov0)
            for t in range(steps):
                f(observations={k: v[t] for k, v in obs.items()}, controls=ctrl[t])
                x, lw = f.particle_states, f.particle_log_weights
                w = torch.softmax(lw, dim=1)
                dx = x - torch.sum(w[:, :, None] * x, dim=1, keepdim=True)
                torch.einsum("nm,nmi,nmj->nij", w, dx, dx), 1.0 / torch.sum(w * w, dim=1), torch.logsumexp(lw, dim=1)

        stepwise_torch()
        v = [1e6 * _timed(stepwise_torch) / steps for _ in range(reps)]
        out["stepwise_forward_plus_torch"] = {"median_us_per_step": statistics.median(v), "min": min(v), "max": max(v)}
        # K1 alone: the launch path's kernel on a fixed belief, 200 launches between two events
        g = torch.Generator(device=dev).manual_seed(1)
        xs = torch.randn((N, M, d), generator=g, device=dev)
        ll = torch.randn((N, M), generator=g, device=dev)
        u = torch.rand((N,), generator=g, device=dev)
        E = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
        est, so, rec = E(N, d), E(N, M, d), (E(N, d, d), E(N), E(N))
        k1 = {}
        for name, outs in (("off", (None, None, None)), ("on", rec)):
            call = lambda: _abi.pf_reweight_resample_belief(ll, None, xs, u, est, so, None, None, 1, 1.0, cov=outs[0], ess=outs[1],
                                                            log_evidence=outs[2])
            for _ in range(20):
                call()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            vals = []
            for _ in range(reps):
                a.record()
                for _ in range(200):
                    call()
                b.record()
                torch.cuda.synchronize()
                vals.append(1e3 * a.elapsed_time(b) / 200)
            k1[name] = {"median_us_per_launch": statistics.median(vals), "min": min(vals), "max": max(vals)}
        out["k1_back_to_back"] = k1
    return out


def ekf_case(N, T, reps, off_only, dev):
    import bench
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import _abi, engine, synthetic

    d = 3
    torch.manual_seed(0)
    f = mmf.door_models.DoorCrossmodalKalmanFilter().to(dev).eval()
    traj = bench.to_device(synthetic.make_trajectories(state_dim=d, T=T, N=N, seed=5), dev)
    obs = {k: traj[k][1:] for k in ("image", "gripper_pos", "gripper_sensors")}
    ctrl = traj["controls"][1:]
    steps = ctrl.shape[0]
    cov0 = (torch.eye(d, device=dev) * 0.1)[None].expand(N, d, d)

    def run(record):
        if record:
            f.record_belief = True
        f.initialize_beliefs(mean=traj["states"][0], covariance=cov0)
        f.forward_loop(observations=obs, controls=ctrl)
        if record:
            f.record_belief = False

    return {"filter": "DoorCrossmodalKalmanFilter", "batch": N, "steps": steps,
            "persistent_eligible": bool(engine.EKF_PERSISTENT and _abi.ekf_persistent_plan(N, 2) > 0),
            "forward_loop": _legs(run, reps, off_only, steps)}


def main():
    ap = bc.arg_parser(__doc__)
    ap.set_defaults(reps=3)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--off-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    doc = {"pf": [pf_case(N, M, args.steps, args.reps, args.off_only, dev) for N, M in ((32, 300), (32, 4096), (256, 4096))],
           "ekf": [ekf_case(N, args.steps, args.reps, args.off_only, dev) for N in (32, 256)]}
    bc.write_document(doc, args.out)


if __name__ == "__main__":
    main()
