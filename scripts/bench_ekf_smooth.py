"""What RTS smoothing of an extended Kalman filter costs (profiles/ekf_smooth/README.md): ``smooth()`` on the history of the
door ``KalmanFilter`` at 32 x T = 100 and 2048 x T = 100, split into its Jacobian recompute (one batched K5 call over the
``(T - 1) N`` recorded means) and ``mmf_ekf_smooth`` (gains, then the serial sweep), next to the ``forward_loop`` that
produced the history, in the same process.  Device time from HIP events around each call, after a warm-up call, median of
``--reps`` calls, the legs alternating.  The two kernels inside ``mmf_ekf_smooth`` are one C call, so their split comes
from ``rocprofv3 --kernel-trace --stats`` on a child process that only smooths (skipped where ``rocprofv3`` is absent).

    python scripts/bench_ekf_smooth.py [--reps 7] [--out FILE]

One JSON document.
"""
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

import torch

import _bench_common as bc

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = ((32, 100), (2048, 100))


def _setup(N, T, dev):
    import bench
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import synthetic

    d = 3
    torch.manual_seed(0)
    f = mmf.model_types("door")["DoorKalmanFilter"]().to(dev).eval()
    synthetic.stabilise_dynamics(f)
    traj = bench.to_device(synthetic.make_trajectories(state_dim=d, T=T, N=N, seed=5), dev)
    obs = {k: traj[k][1:] for k in ("image", "gripper_pos", "gripper_sensors")}
    cov = (torch.eye(d, device=dev) * 0.1)[None].expand(N, d, d)

    def forward(record):
        f.record_history = record
        f.initialize_beliefs(mean=traj["states"][0], covariance=cov)
        return f.forward_loop(observations=obs, controls=traj["controls"][1:])

    return f, d, forward


def case(N, T, reps, dev):
    from multimodalfilter_amd import _abi

    f, d, forward = _setup(N, T, dev)
    forward(True)
    h = f.last_history
    assert h.means.shape == (T, N, d)
    with torch.no_grad():
        pred, A, L = f._smoothing_transition(h)
    E = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    mean, cov, gain, Pp, e, m2 = E(T, N, d), E(T, N, d, d), E(T - 1, N, d, d), E(T - 1, N, d, d), E(T - 1, N, d), E(T - 1, N, d, d)

    def smooth(lag=None, moments=False):  # always on the history taken above, whatever leg ran before
        f.last_history, f.record_transition_moments = h, moments
        try:
            return f.smooth(lag)
        finally:
            f.record_transition_moments = False

    runs = {"forward_loop": lambda: forward(False),
            "forward_loop_recording": lambda: forward(True),
            "smooth": smooth,                                               # the recompute and mmf_ekf_smooth
            "smooth_with_moments": lambda: smooth(moments=True),
            "smooth_lag_5": lambda: smooth(5),
            "jacobian_recompute": lambda: f._smoothing_transition(h),
            "mmf_ekf_smooth": lambda: _abi.ekf_smooth(h.means, h.covariances, A, pred, L, None, mean, cov, gain, Pp),
            "mmf_ekf_smooth_with_moments": lambda: _abi.ekf_smooth(h.means, h.covariances, A, pred, L, None, mean, cov, gain, Pp, e, m2),
            "mmf_ekf_smooth_lag_5": lambda: _abi.ekf_smooth(h.means, h.covariances, A, pred, L, 5, mean, cov, gain, Pp)}
    with torch.no_grad():
        times = bc.time_alternating(runs, reps)
    med = {k: statistics.median(v) for k, v in times.items()}
    return {"filter": "DoorKalmanFilter", "batch": N, "steps": T, "state_dim": d,
            "history_bytes": 4 * (d * d + d) * T * N, "workspace_bytes": 2 * 4 * d * d * (T - 1) * N,
            "ms_per_call": {k: bc.stats(v) for k, v in times.items()},
            "smooth_over_forward_loop": med["smooth"] / med["forward_loop"],
            "recording_over_plain_forward_loop": med["forward_loop_recording"] / med["forward_loop"]}


def leg(N, T, reps, dev):
    """The child under the profiler: one forward loop, then ``reps + 1`` full smooths with moments (the first one cold)."""
    f, d, forward = _setup(N, T, dev)
    forward(True)
    f.record_transition_moments = True
    for _ in range(reps + 1):
        f.smooth()
    torch.cuda.synchronize()
    print(json.dumps({"N": N, "T": T, "reps": reps}))


def kernel_split(N, T, reps):
    """Average device time of the kernels behind ``mmf_ekf_smooth`` (and of the K5 launch of the recompute) from
    ``rocprofv3 --kernel-trace --stats`` on a child that smooths ``reps + 1`` times; the slowest call of each kernel (the
    cold first one) is left out of the average."""
    if shutil.which("rocprofv3") is None:
        return None
    out = tempfile.mkdtemp(prefix="bench_ekf_smooth_prof_")
    cmd = ["timeout", "-k", "10", "420", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "run",
           "--", sys.executable, os.path.abspath(__file__), "--leg", "--N", str(N), "--T", str(T), "--reps", str(reps)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    stats = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    rows = {}
    if stats:
        with open(stats[0]) as fh:
            for row in csv.DictReader(fh):
                name = row.get("Name", "")
                for key in ("ekf_smooth_gains_kernel", "ekf_smooth_sweep_kernel"):
                    if key in name:
                        calls = int(float(row.get("Calls") or 0))
                        total, worst = float(row.get("TotalDurationNs") or 0), float(row.get("MaxNs") or 0)
                        rows[key] = {"calls": calls, "average_us_without_slowest": (total - worst) / max(calls - 1, 1) * 1e-3,
                                     "min_us": float(row.get("MinNs") or 0) * 1e-3, "max_us": worst * 1e-3}
    shutil.rmtree(out, ignore_errors=True)
    return {"batch": N, "steps": T, "kernels": rows} if rows else None


def main():
    ap = bc.arg_parser(__doc__)
    ap.add_argument("--leg", action="store_true")
    ap.add_argument("--N", type=int, default=32)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--no-profile", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.leg:
        leg(args.N, args.T, args.reps, dev)
        return
    doc = {"device": torch.cuda.get_device_name(0), "cases": [case(N, T, args.reps, dev) for N, T in SIZES]}
    if not args.no_profile:
        doc["kernel_split"] = [kernel_split(N, T, args.reps) for N, T in SIZES]
    bc.write_document(doc, args.out)


if __name__ == "__main__":
    main()
