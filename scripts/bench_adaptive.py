"""What ESS-triggered resampling costs (profiles/adaptive/README.md): ``forward_loop`` of the door crossmodal particle filter
with ``resample_ess_threshold`` unset and at 0.5, alternating, at 32 x 300 (the persistent launch) and 256 x 4096 (the loop of
launches), on measurement heads calibrated so that the weights do degenerate (``synthetic.calibrate_measurement_heads``).

    python scripts/bench_adaptive.py [--reps 5] [--steps 64] [--unset-only] [--out FILE]

One JSON document.  ``--unset-only`` touches nothing this feature added, so the same file runs on the parent commit.
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


def pf_case(N, M, T, reps, unset_only, dev):
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import _abi, engine

    door = bc.recorded_door_run(N, M, T + 1, dev, run=False)
    f, traj, obs, ctrl, cov0 = door.f, door.traj, door.obs, door.ctrl, door.cov0
    f.reserve(steps=T, batch=N, particles=M)
    settings = [None] if unset_only else [None, 0.5]
    shares = {}

    def run(thr):
        if thr is not None:
            f.resample_ess_threshold = thr
        f.noise = mmf.CounterNoise(7)
        f.initialize_beliefs(mean=traj["states"][0], covariance=cov0)
        f.forward_loop(observations=obs, controls=ctrl)
        if thr is not None:
            shares[thr] = float(f.last_resampled.float().mean())
            f.resample_ess_threshold = None

    for thr in settings:
        run(thr)  # warm-up: allocator, packed-weight caches, code objects
    times = {thr: [] for thr in settings}
    for _ in range(reps):
        for thr in settings:  # alternating
            times[thr].append(1e6 * _timed(lambda: run(thr)) / T)
    legs = {("unset" if thr is None else str(thr)): {"median_us_per_step": statistics.median(v), "min": min(v), "max": max(v)}
            for thr, v in times.items()}
    for thr, s in shares.items():
        legs[str(thr)]["share_of_trajectory_steps_resampling"] = s
    return {"filter": "DoorCrossmodalParticleFilter", "batch": N, "particles": M, "steps": T,
            "persistent_eligible": bool(engine.PF_PERSISTENT and _abi.pf_persistent_plan(N, M, 2) > 0),
            "forward_loop": legs}


def main():
    ap = bc.arg_parser(__doc__)
    ap.set_defaults(reps=5)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--unset-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    doc = {"pf": [pf_case(N, M, args.steps, args.reps, args.unset_only, dev) for N, M in ((32, 300), (256, 4096))]}
    bc.write_document(doc, args.out)


if __name__ == "__main__":
    main()
