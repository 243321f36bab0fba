"""What particle smoothing costs (profiles/smooth/README.md): ``forward_loop`` of the door crossmodal particle filter with
``record_history`` off and on, alternating, and ``smooth()`` at lag 0, lag 10 and the full smoother on the recorded history,
at 32 x 300 and 256 x 4096, on measurement heads calibrated so that the weights do degenerate.

    python scripts/bench_smooth.py [--reps 5] [--steps 300] [--off-only] [--out FILE]

One JSON document.  ``--off-only`` touches nothing this feature added, so the same file runs on the parent commit; with
``record_history`` off the loop is the parent's (the persistent launch at 32 x 300), with it on it is the loop of launches.
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


def pf_case(N, M, T, reps, off_only, dev):
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import _abi, engine

    door = bc.recorded_door_run(N, M, T + 1, dev, run=False)
    f, traj, obs, ctrl, cov0, d = door.f, door.traj, door.obs, door.ctrl, door.cov0, door.dims[3]
    if not off_only:
        f.record_history = True  # reserve() accounts for the history arrays
    f.reserve(steps=T, batch=N, particles=M)
    settings = [False] if off_only else [False, True]

    def run(history):
        if not off_only:
            f.record_history = history
        f.noise = mmf.CounterNoise(7)
        f.initialize_beliefs(mean=traj["states"][0], covariance=cov0)
        return f.forward_loop(observations=obs, controls=ctrl)

    est = {h: run(h) for h in settings}  # warm-up: allocator, packed-weight caches, code objects
    times = {h: [] for h in settings}
    for _ in range(reps):
        for h in settings:  # alternating
            times[h].append(1e6 * _timed(lambda: run(h)) / T)
    doc = {"filter": "DoorCrossmodalParticleFilter", "batch": N, "particles": M, "steps": T,
           "persistent_eligible": bool(engine.PF_PERSISTENT and _abi.pf_persistent_plan(N, M, 2) > 0),
           "forward_loop_us_per_step": {("record_history" if h else "off"): bc.stats(v) for h, v in times.items()}}
    if off_only:
        return doc
    doc["estimates_identical_bits"] = bool(torch.equal(est[False], est[True]))
    doc["history_bytes"] = 4 * (d + 3) * N * M * T
    smooth = {}
    for name, lag in (("lag_0", 0), ("lag_10", 10), ("full", None)):
        f.smooth(lag)  # warm-up
        v = [1e3 * _timed(lambda: f.smooth(lag)) for _ in range(reps)]
        uniq = f.last_smoothed.unique.float()
        smooth[name] = {"ms_per_call": bc.stats(v), "us_per_step": statistics.median(v) * 1e3 / T,
                        "mean_unique_first_step": float(uniq[0].mean()), "mean_unique_last_step": float(uniq[-1].mean())}
    doc["smooth"] = smooth
    return doc


def main():
    ap = bc.arg_parser(__doc__)
    ap.set_defaults(reps=5)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--off-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    doc = {"pf": [pf_case(N, M, args.steps, args.reps, args.off_only, dev) for N, M in ((32, 300), (256, 4096))]}
    bc.write_document(doc, args.out)


if __name__ == "__main__":
    main()
