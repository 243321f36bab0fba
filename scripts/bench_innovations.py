"""What recording the innovations of a Kalman filter costs (profiles/innovations/README.md): ``forward_loop`` of the door
``CrossmodalKalmanFilter`` at the reference's evaluation size (32 trajectories, T = 100) three ways, in one process:

  persistent          today's default: the whole loop as ONE persistent launch
  loop_of_launches    the persistent form switched off (``engine.persistent_forms(ekf=False)``, the switch that
                      ``MMF_EKF_PERSISTENT=0`` sets from the start): 2 T launches
  loop_recording      ``record_innovations`` set: the loop of launches with the innovation step (``mmf_ekf_step_innov``),
                      which is what the switch takes in place of the persistent launch

A sample is the host time of ``--calls`` consecutive ``forward_loop`` calls that end in a device synchronise, divided by
their number; after a warm-up of every leg, ``--reps`` samples per leg, the legs alternating.  The estimates of the three legs
are compared bit for bit before anything is timed.  ``recording_cost`` is against the loop of launches, next to that loop's
own run-to-run spread; ``recording_over_persistent`` is what a user who sets the switch pays against the default.

    python scripts/bench_innovations.py [--reps 15] [--calls 20] [--out FILE]

One JSON document.  Needs the GPU: there is no CPU path to time.
"""
import os
import statistics
import sys
import time

import torch

import _bench_common as bc

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, T, D = 32, 100, 3


def main():
    ap = bc.arg_parser(__doc__)
    ap.set_defaults(reps=15)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_innovations: no GPU; a time is measured on the device or not at all")
    dev = torch.device("cuda:0")

    import bench
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import engine, synthetic

    torch.manual_seed(0)
    f = mmf.model_types("door")["DoorCrossmodalKalmanFilter"]().to(dev).eval()
    synthetic.stabilise_dynamics(f)
    traj = bench.to_device(synthetic.make_trajectories(state_dim=D, T=T, N=N, seed=5), dev)
    obs = {k: traj[k][1:] for k in ("image", "gripper_pos", "gripper_sensors")}
    cov = (torch.eye(D, device=dev) * 0.1)[None].expand(N, D, D)

    def forward(record, persistent):
        f.record_innovations = record
        f.initialize_beliefs(mean=traj["states"][0], covariance=cov)
        with engine.persistent_forms(ekf=persistent):
            return f.forward_loop(observations=obs, controls=traj["controls"][1:])

    legs = {"persistent": lambda: forward(False, True),
            "loop_of_launches": lambda: forward(False, False),
            "loop_recording": lambda: forward(True, False)}
    with torch.no_grad():
        first = {k: fn() for k, fn in legs.items()}  # warm-up of every leg: code objects, allocator, packed weights
        torch.cuda.synchronize()
        same = {k: bool(torch.equal(first[k], first["loop_of_launches"])) for k in legs}
        record = f.last_innovations
        assert record is not None and record.nis.shape == (T, 2, N), "the recording leg left no record"
        times = {k: [] for k in legs}
        for _ in range(args.reps):
            for k, fn in legs.items():  # alternating
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    fn()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) * 1e3 / args.calls)
    f.record_innovations = False
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = max(times["loop_of_launches"]) - min(times["loop_of_launches"])
    cost = med["loop_recording"] - med["loop_of_launches"]
    doc = {"device": torch.cuda.get_device_name(0), "filter": "DoorCrossmodalKalmanFilter", "batch": N, "steps": T,
           "sub_filters": 2, "state_dim": D, "calls_per_sample": args.calls, "samples": args.reps,
           "estimates_equal_to_loop_of_launches": same,
           "record_bytes": 3 * 4 * T * 2 * N,
           "ms_per_forward_loop": {k: bc.stats(v) for k, v in times.items()},
           "loop_of_launches_spread_ms": spread,
           "recording_cost_ms": cost,
           "recording_cost_exceeds_spread": bool(cost > spread),
           "recording_over_loop_of_launches": med["loop_recording"] / med["loop_of_launches"],
           "recording_over_persistent": med["loop_recording"] / med["persistent"]}
    bc.write_document(doc, args.out)


if __name__ == "__main__":
    main()
