#!/usr/bin/env python3
"""The LSTM baseline's evaluation cost: a door ``DoorLSTMFilter`` in eval mode through ``evaluation.run_filter`` at
N in {32, 256} trajectories and T = 256 steps, in three forms -- the recurrence as ONE persistent launch, as a loop of
launches (``MMF_LSTM_PERSISTENT=0``), and the same module's torch path on the GPU (``nn.LSTM`` on MIOpen plus torch
encoders: the reference's own eval, ``crossmodal/door_models/lstm.py:62-100``) -- and, from ``rocprofv3 --kernel-trace
--stats``, the recurrence kernel's share of the GPU time of a step.  Prints ONE JSON line.

    python scripts/bench_lstm.py [--T 256] [--reps 5] [--out profiles/lstm/bench_lstm.json]

Every measurement runs in a child process of its own under ``timeout`` (the driver itself never opens the GPU).
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = ("persistent", "launches", "torch")
NS = (32, 256)


def leg(form: str, N: int, T: int, reps: int) -> dict:
    """One measurement (child process): ms per filter step of run_filter, median over ``reps`` timed runs."""
    sys.path.insert(0, ROOT)
    import torch

    from multimodalfilter_amd import engine, evaluation, synthetic
    from multimodalfilter_amd.door_models import DoorLSTMFilter

    dev = torch.device("cuda:0")
    with engine.persistent_forms(lstm=form == "persistent"):
        torch.manual_seed(0)
        model = DoorLSTMFilter().to(dev).eval()
        traj = {k: v.to(dev) for k, v in synthetic.make_trajectories(state_dim=3, T=T, N=N, seed=1).items()}
        if form == "torch":
            def run():
                with torch.no_grad():
                    obs = {k: traj[k][1:] for k in ("image", "gripper_pos", "gripper_sensors")}
                    hidden = (torch.zeros(2, N, 512, device=dev), torch.zeros(2, N, 512, device=dev))
                    feat = model.observation_image_layers(obs["image"].reshape(T * N, 1, 32, 32)).reshape(T, N, 64)
                    merged = torch.cat((feat, model.observation_pos_layers(obs["gripper_pos"]),
                                        model.observation_sensors_layers(obs["gripper_sensors"]),
                                        model.control_layers(traj["controls"][1:])), dim=-1)
                    out, _ = model.lstm(model.fusion_layers(merged), hidden)
                    return model.output_layers(out)
        else:
            def run():
                return evaluation.run_filter(model, traj)
        for _ in range(2):
            run()
        torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            run()
            e.record()
            torch.cuda.synchronize()
            times.append(s.elapsed_time(e))
    times.sort()
    return {"form": form, "N": N, "T": T, "ms_per_step": times[len(times) // 2] / T,
            "ms_per_step_min": times[0] / T, "reps": reps}


def child(args, form, N, timeout_s=300, prefix=()):
    cmd = ["timeout", "-k", "10", str(timeout_s), *prefix, sys.executable, os.path.abspath(__file__), "--leg", form,
           "--N", str(N), "--T", str(args.T), "--reps", str(args.reps)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    return json.loads([line for line in p.stdout.splitlines() if line.startswith("{")][-1])


def kernel_share(args, N):
    """rocprofv3 kernel stats of the persistent leg: the recurrence kernel's share of all kernel time."""
    if shutil.which("rocprofv3") is None:
        return None
    out = tempfile.mkdtemp(prefix="bench_lstm_prof_")
    child(args, "persistent", N, 600, ("rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "run", "--"))
    stats = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    if not stats:
        return None
    total, lstm, pack = 0.0, 0.0, 0.0
    with open(stats[0]) as fh:
        for row in csv.DictReader(fh):
            ns = float(row.get("TotalDurationNs") or 0)
            total += ns
            if "lstm_rounds_kernel" in row.get("Name", ""):
                lstm += ns
            if "lstm_pack_kernel" in row.get("Name", ""):
                pack += ns
    shutil.rmtree(out, ignore_errors=True)
    return {"N": N, "lstm_kernel_share_of_gpu_time": lstm / total if total else None, "lstm_kernel_ms": lstm * 1e-6,
            "all_kernels_ms": total * 1e-6, "runs_profiled": args.reps + 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=FORMS)
    ap.add_argument("--N", type=int, default=32)
    ap.add_argument("--T", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.leg:
        print(json.dumps(leg(args.leg, args.N, args.T, args.reps)))
        return
    result = {"bench": "lstm_eval", "task": "door", "T": args.T, "legs": {}}
    for N in NS:
        for form in FORMS:
            r = child(args, form, N)
            result["legs"][f"{form}_N{N}"] = r["ms_per_step"]
        result["legs"][f"persistent_vs_launches_N{N}"] = (result["legs"][f"persistent_N{N}"] / result["legs"][f"launches_N{N}"])
    if not args.no_profile:
        result["profile"] = [kernel_share(args, N) for N in NS]
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
