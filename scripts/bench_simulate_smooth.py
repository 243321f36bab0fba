"""What backward-simulation particle smoothing costs (profiles/simulate_smooth/README.md): ``smooth(method="simulation")`` with
``S = 64`` draws on the history of the door crossmodal particle filter at 32 x 300 x T = 100 and 32 x 4096 x T = 20, next to a
torch-ops statement of the same recursion on the same history, predictions and uniforms, and next to
``smooth(method="marginal")`` on that history.  Device time from HIP events around each call, after a warm-up call, median of
``--reps`` calls, the implementations alternating.

    python scripts/bench_simulate_smooth.py [--reps 7] [--out FILE]

One JSON document.  ``densities`` counts the transition densities the recursion evaluates, ``(T - 1) N S M``.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DRAWS = 64


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def _stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def torch_simulate(X, F, ll, lw, L, u):
    """The recursion of ``include/mmf.h`` ("backward-simulation particle smoothing") in torch ops: per step the ``(N, S, M)``
    table of ``log W_t[i] + lp_t[i, j_{t+1}]`` (difference first, then the triangular solve), its exponentials about the row
    maximum, a ``cumsum`` over the particles and a ``searchsorted`` of ``u * total``.  The finite log-weights of a benchmark
    run need no dead-particle handling."""
    T, N, M, d = X.shape
    S = u.shape[2]
    a = ll + lw
    Linv_t = torch.linalg.inv(L).t().contiguous()
    idx = torch.empty((T, N, S), dtype=torch.int64, device=X.device)
    paths = torch.empty((T, N, S, d), dtype=torch.float32, device=X.device)
    for t in range(T - 1, -1, -1):
        v = a[t][:, None, :]
        if t < T - 1:
            z = (paths[t + 1][:, :, None, :] - F[t][:, None, :, :]) @ Linv_t
            v = v - 0.5 * (z * z).sum(-1)
        v = v.expand(N, S, M)
        c = torch.cumsum(torch.exp(v - v.max(-1, keepdim=True).values), dim=-1)
        j = torch.searchsorted(c, (u[t] * c[..., -1])[..., None], right=True)[..., 0].clamp_(max=M - 1)
        idx[t] = j
        paths[t] = torch.gather(X[t], 1, j[..., None].expand(N, S, d))
    mean = paths.mean(2)
    dx = paths - mean[:, :, None, :]
    return idx, paths, mean, torch.einsum("tnsi,tnsj->tnij", dx, dx) / S


def case(N, M, T, reps, dev):
    import bench
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import _abi, synthetic

    d, S = 3, DRAWS
    torch.manual_seed(0)
    f = mmf.door_models.DoorCrossmodalParticleFilter().to(dev).eval()
    synthetic.stabilise_dynamics(f)
    traj = bench.to_device(synthetic.make_trajectories(state_dim=d, T=T, N=N, seed=5), dev)
    obs = {k: traj[k][1:] for k in ("image", "gripper_pos", "gripper_sensors")}
    ctrl = traj["controls"][1:]
    cal = traj["states"][0][:, None, :] + 0.3 * torch.randn((N, 256, d), device=dev)
    synthetic.calibrate_measurement_heads(f, {k: v[0] for k, v in obs.items()}, cal)
    f.num_particles = M
    f.record_history = True
    f.noise = mmf.CounterNoise(7)
    f.initialize_beliefs(mean=traj["states"][0], covariance=(torch.eye(d, device=dev) * 0.1)[None].expand(N, d, d))
    f.forward_loop(observations=obs, controls=ctrl)
    h = f.last_history
    assert h.states.shape == (T, N, M, d)
    dyn = f.dynamics_model
    L = dyn.scale_tril().detach().float().contiguous()
    with torch.no_grad():
        ctx = dyn.encode_controls(ctrl[1:].reshape((T - 1) * N, -1))
        F = dyn.propagate_encoded(h.states[:-1].reshape((T - 1) * N, M, d), ctx, None).reshape(T - 1, N, M, d)
    u = torch.rand((T, N, S), generator=torch.Generator().manual_seed(11)).to(dev)
    idx = torch.empty((T, N, S), dtype=torch.int32, device=dev)
    paths = torch.empty((T, N, S, d), device=dev)
    mean, cov = torch.empty((T, N, d), device=dev), torch.empty((T, N, d, d), device=dev)

    class Replay(mmf.NoiseSource):  # the same (T, N, S) uniforms at every call of smooth(method="simulation")
        def uniform(self, shape, *, like):
            assert tuple(shape) == tuple(u.shape)
            return u

    f.noise = Replay()

    def hip_recursion():
        _abi.pf_smooth_simulate(h.states, F, h.log_likelihoods, h.log_weights_in, L, u, idx, paths, mean, cov)
        return idx, paths, mean, cov

    runs = {"smooth_simulation": lambda: f.smooth(method="simulation", num_draws=S),  # the prediction F and the recursion
            "hip_recursion": hip_recursion,                                           # mmf_pf_smooth_simulate alone, F given
            "torch_recursion": lambda: torch_simulate(h.states, F, h.log_likelihoods, h.log_weights_in, L, u),
            "smooth_marginal": lambda: f.smooth(method="marginal")}
    with torch.no_grad():
        out = {k: fn() for k, fn in runs.items()}  # warm-up: code objects, allocator
        torch.cuda.synchronize()
        marginal_mean, marginal_cov = out["smooth_marginal"].clone(), f.last_smoothed.covariance.clone()
        hip = [x.clone() for x in out["hip_recursion"]]
        times = {k: [] for k in runs}
        for _ in range(reps):
            for k, fn in runs.items():  # alternating
                times[k].append(_event_ms(fn)[0])

    ref = out["torch_recursion"]
    densities = float(T - 1) * N * S * M
    med = {k: statistics.median(v) for k, v in times.items()}
    # the two samplers round differently: a draw on a boundary of the CDF takes the neighbouring particle and the path
    # parts from there, so whole paths are compared by their share; the means are held to the marginal smoother's
    # (the tests' bound is 5 standard errors + 1e-4: where the smoothed weights sit on one particle there is no spread)
    stderr = (torch.diagonal(marginal_cov, dim1=-2, dim2=-1) / S).sqrt() + 1e-4 / 5
    return {"filter": "DoorCrossmodalParticleFilter", "batch": N, "particles": M, "steps": T, "state_dim": d, "draws": S,
            "densities": densities, "marginal_pairs": 2.0 * (T - 1) * N * M * M, "prediction_bytes": 4 * d * (T - 1) * N * M,
            "ms_per_call": {k: _stats(v) for k, v in times.items()},
            "densities_per_second": {k: densities / (1e-3 * med[k]) for k in ("hip_recursion", "torch_recursion")},
            "torch_over_hip": med["torch_recursion"] / med["hip_recursion"],
            "marginal_over_simulation": med["smooth_marginal"] / med["smooth_simulation"],
            "hip_against_torch": {"share_of_equal_indices": float((hip[0].long() == ref[0]).float().mean()),
                                  "share_of_equal_whole_paths": float((hip[0].long() == ref[0]).all(0).float().mean())},
            "worst_mean_minus_marginal_mean_in_standard_errors": {
                "hip": float(((hip[2] - marginal_mean).abs() / stderr).max()),
                "torch": float(((ref[2] - marginal_mean).abs() / stderr).max())},
            "dead_draws": int((hip[0] < 0).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    doc = {"device": torch.cuda.get_device_name(0),
           "cases": [case(N, M, T, args.reps, dev) for N, M, T in ((32, 300, 100), (32, 4096, 20))]}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
