"""What backward-simulation particle smoothing costs (profiles/simulate_smooth/README.md): ``smooth(method="simulation")`` with
``S = 64`` draws on the history of the door crossmodal particle filter at 32 x 300 x T = 100 and 32 x 4096 x T = 20, next to a
torch-ops statement of the same recursion on the same history, predictions and uniforms, and next to
``smooth(method="marginal")`` on that history.  Device time from HIP events around each call, after a warm-up call, median of
``--reps`` calls, the implementations alternating.

    python scripts/bench_simulate_smooth.py [--reps 7] [--out FILE]

One JSON document.  ``densities`` counts the transition densities the recursion evaluates, ``(T - 1) N S M``.
"""
import os
import statistics
import sys

import torch

import _bench_common as bc

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DRAWS = 64


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
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import _abi

    door = bc.recorded_door_run(N, M, T, dev)
    f, h, ctrl, d = door.f, door.f.last_history, door.ctrl, door.dims[3]
    S = DRAWS
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
        times = bc.time_alternating(runs, reps)
        out = {k: fn() for k, fn in runs.items()}  # (smooth_marginal last: last_smoothed is its record)
        marginal_mean, marginal_cov = out["smooth_marginal"], f.last_smoothed.covariance
        hip = out["hip_recursion"]

    ref = out["torch_recursion"]
    densities = float(T - 1) * N * S * M
    med = {k: statistics.median(v) for k, v in times.items()}
    # the two samplers round differently: a draw on a boundary of the CDF takes the neighbouring particle and the path
    # parts from there, so whole paths are compared by their share; the means are held to the marginal smoother's
    # (the tests' bound is 5 standard errors + 1e-4: where the smoothed weights sit on one particle there is no spread)
    stderr = (torch.diagonal(marginal_cov, dim1=-2, dim2=-1) / S).sqrt() + 1e-4 / 5
    return {"filter": "DoorCrossmodalParticleFilter", "batch": N, "particles": M, "steps": T, "state_dim": d, "draws": S,
            "densities": densities, "marginal_pairs": 2.0 * (T - 1) * N * M * M, "prediction_bytes": 4 * d * (T - 1) * N * M,
            "ms_per_call": {k: bc.stats(v) for k, v in times.items()},
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
    args = bc.arg_parser(__doc__).parse_args()
    dev = torch.device("cuda:0")
    doc = {"device": torch.cuda.get_device_name(0),
           "cases": [case(N, M, T, args.reps, dev) for N, M, T in ((32, 300, 100), (32, 4096, 20))]}
    bc.write_document(doc, args.out)


if __name__ == "__main__":
    main()
