"""What the particle-posterior distances cost (profiles/distance/README.md): ``belief_distance`` on the history of the door
crossmodal particle filter -- the filtered against the marginal-smoothed sets at 32 x 300 x T = 100 and 32 x 4096 x T = 20, and
a 300-particle against a 4096-particle run of the same model on the same data (T = 20) --, ``mmf_pf_distance`` alone on the
same tensors (all five outputs, the CDF kernel alone, the pair kernel alone), and the formulation a caller would write today
in torch ops on the same device: per dimension ``cat`` + ``sort`` + two gathered ``cumsum``s over the union of both sets, and
for the energy distance three ``torch.cdist`` contracted with the weights by ``bmm``, over chunks of rows sized so that a
chunk's ``(rows, Ma, Mb)`` array stays within 256 MiB.  Device time from HIP events around each call, after a warm-up call of
each, median / min / max of ``--reps`` calls, the formulations alternating.

    python scripts/bench_distance.py [--reps 7] [--out FILE]

One JSON document.  ``pairs``: ``R (Ma Mb + Ma^2 + Mb^2)`` per call, what both formulations of the energy distance visit.
``max_abs_difference`` / ``max_rel_difference``: the largest element-wise difference between the kernels and the torch
formulation per output (relative: against ``max(|value|, 1e-3 x the output's largest)``); ``hip_against_fp64`` /
``torch_ops_against_fp64``: the same figures of either against the torch formulation in fp64 on ``fp64_row_pairs`` evenly
spaced row pairs, which says which of the two is off where they differ (the fp64 formulation keeps plain weights, so on the
CDF outputs it is the ``2^-24`` truncation of the kernel's fixed-point weights away from the kernel's definition)."""
import os
import statistics
import sys

import torch

import _bench_common as bc

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CHUNK_BYTES = 256 << 20


def _flat(sets):
    """``(states (T, N, M, d), log_a, log_b (T, N, M) or None)`` with the two leading axes merged."""
    return tuple(None if x is None else x.reshape((-1,) + tuple(x.shape[2:])) for x in sets)


def _weights(states, log_a, log_b, dtype=torch.float32):
    """Normalised weights ``(R, M)`` and the states with dead particles (weight 0, NaN rows) zeroed, ``(R, M, d)``, in ``dtype``."""
    R, M, d = states.shape
    a = torch.zeros((R, M), device=states.device) if log_a is None and log_b is None else (
        log_a if log_b is None else log_b if log_a is None else log_a + log_b)
    W = torch.softmax(a.to(dtype), dim=-1)
    X = torch.where((W > 0)[..., None], states.to(dtype), torch.zeros((), dtype=dtype, device=states.device))
    return W, X


def torch_cdf(Wa, Xa, Wb, Xb):
    """``wasserstein, cramer, ks (R, d)`` in torch ops of the inputs' precision: the union of both sets sorted per dimension,
    the two CDFs as cumulative sums of the gathered weights.  (A dead particle sits at 0 with weight 0: a point of the union that moves
    neither CDF.)"""
    R, Ma, d = Xa.shape
    Mb = Xb.shape[1]
    z, order = torch.sort(torch.cat([Xa, Xb], dim=1), dim=1)
    wa = torch.cat([Wa, torch.zeros((R, Mb), dtype=Wa.dtype, device=Wa.device)], dim=1)[..., None].expand(R, Ma + Mb, d)
    wb = torch.cat([torch.zeros((R, Ma), dtype=Wa.dtype, device=Wa.device), Wb], dim=1)[..., None].expand(R, Ma + Mb, d)
    D = (torch.cumsum(torch.gather(wa, 1, order), dim=1) - torch.cumsum(torch.gather(wb, 1, order), dim=1))[:, :-1]
    gap = z[:, 1:] - z[:, :-1]
    absD = D.abs()
    return (gap * absD).sum(1), (gap * D * D).sum(1), torch.where(gap > 0, absD, torch.zeros_like(absD)).amax(1)


def torch_energy(Wa, Xa, Wb, Xb):
    """``energy (R)``, ``terms (R, 3)`` in torch ops of the inputs' precision: three ``torch.cdist`` contracted with the weights."""
    R, Ma, _ = Xa.shape
    Mb = Xb.shape[1]
    terms = torch.empty((R, 3), dtype=Xa.dtype, device=Xa.device)
    rows = max(1, CHUNK_BYTES // (Xa.element_size() * max(Ma, Mb) ** 2))
    for c in range(0, R, rows):
        xa, xb, wa, wb = Xa[c:c + rows], Xb[c:c + rows], Wa[c:c + rows], Wb[c:c + rows]
        terms[c:c + rows, 0] = (wa[:, None, :] @ torch.cdist(xa, xb) @ wb[:, :, None])[:, 0, 0]
        terms[c:c + rows, 1] = (wa[:, None, :] @ torch.cdist(xa, xa) @ wa[:, :, None])[:, 0, 0]
        terms[c:c + rows, 2] = (wb[:, None, :] @ torch.cdist(xb, xb) @ wb[:, :, None])[:, 0, 0]
    return torch.sqrt((2 * terms[:, 0] - terms[:, 1] - terms[:, 2]).clamp_min(0)), terms


def case(what, N, Ma, Mb, T, reps, dev):
    from multimodalfilter_amd import _abi

    d = 3
    fa = bc.recorded_door_run(N, Ma, T, dev).f
    if what == "filtered_vs_marginal_smoothed":
        assert Ma == Mb
        fb, kw = fa, dict(of="filtered", other_of="smoothed")
        fa.smooth(method="marginal")
    else:
        fb, kw = bc.recorded_door_run(N, Mb, T, dev).f, dict(of="filtered", other_of="filtered")
    a, b = fa._recorded_sets(kw["of"], "bench"), fb._recorded_sets(kw["other_of"], "bench")
    fa_, fb_ = _flat(a), _flat(b)
    new = lambda *tail: torch.empty((T, N) + tail, dtype=torch.float32, device=dev)
    out = dict(wasserstein=new(d), cramer=new(d), ks=new(d), energy=new(), terms=new(3))
    cdf = {k: out[k] for k in ("wasserstein", "cramer", "ks")}
    pairs_out = {k: out[k] for k in ("energy", "terms")}

    def torch_all():
        Wa, Xa = _weights(*fa_)
        Wb, Xb = _weights(*fb_)
        return torch_cdf(Wa, Xa, Wb, Xb) + torch_energy(Wa, Xa, Wb, Xb)

    def torch_cdf_only():
        Wa, Xa = _weights(*fa_)
        Wb, Xb = _weights(*fb_)
        return torch_cdf(Wa, Xa, Wb, Xb)

    def torch_energy_only():
        Wa, Xa = _weights(*fa_)
        Wb, Xb = _weights(*fb_)
        return torch_energy(Wa, Xa, Wb, Xb)

    runs = {"belief_distance": lambda: fa.belief_distance(fb, **kw),
            "hip_distance": lambda: _abi.pf_distance(*a, *b, **out),                 # mmf_pf_distance alone: all five outputs
            "hip_cdf_only": lambda: _abi.pf_distance(*a, *b, **cdf),                 # the CDF kernel
            "hip_pairs_only": lambda: _abi.pf_distance(*a, *b, **pairs_out),         # the pair kernel(s)
            "torch_ops": torch_all, "torch_cdf_only": torch_cdf_only, "torch_energy_only": torch_energy_only}
    with torch.no_grad():
        times = bc.time_alternating(runs, reps)
        runs["hip_distance"]()
        t_w, t_c, t_ks, t_energy, t_terms = torch_all()
        # which of the two is off where they differ: both against the same torch ops in fp64, on every STRIDE-th row pair
        R = T * N
        sub = torch.arange(0, R, max(1, R // 64), device=dev)
        cut = lambda sets: tuple(None if x is None else x[sub] for x in sets)
        Wa, Xa = _weights(*cut(fa_), dtype=torch.float64)
        Wb, Xb = _weights(*cut(fb_), dtype=torch.float64)
        want = dict(zip(("wasserstein", "cramer", "ks", "energy", "terms"), torch_cdf(Wa, Xa, Wb, Xb) + torch_energy(Wa, Xa, Wb, Xb)))
        torch.cuda.synchronize()
    med = {k: statistics.median(x) for k, x in times.items()}
    pairs = float(R) * (Ma * Mb + Ma * Ma + Mb * Mb)
    flat = lambda x: x.reshape((R,) + tuple(x.shape[2:]))
    torch32 = dict(wasserstein=t_w, cramer=t_c, ks=t_ks, energy=t_energy, terms=t_terms)
    return {"what": what, "filter": "DoorCrossmodalParticleFilter", "batch": N, "particles": [Ma, Mb], "steps": T, "state_dim": d,
            "row_pairs": R, "pairs": pairs, "cdf_workgroups": R * d, "lds_bytes_per_cdf_workgroup": _abi.pf_distance_lds_bytes(Ma, Mb),
            "workspace_bytes": _abi.pf_distance_workspace_bytes(R, Ma, Mb, d),
            "torch_rows_per_chunk": max(1, CHUNK_BYTES // (4 * max(Ma, Mb) ** 2)),
            "ms_per_call": {k: bc.stats(x) for k, x in times.items()},
            "torch_over_hip": med["torch_ops"] / med["hip_distance"],
            "torch_over_hip_cdf": med["torch_cdf_only"] / med["hip_cdf_only"],
            "torch_over_hip_pairs": med["torch_energy_only"] / med["hip_pairs_only"],
            "hip_pairs_per_second": pairs / (1e-3 * med["hip_pairs_only"]),
            "torch_pairs_per_second": pairs / (1e-3 * med["torch_energy_only"]),
            "difference": {"wasserstein": bc.max_difference(flat(out["wasserstein"]), t_w), "cramer": bc.max_difference(flat(out["cramer"]), t_c),
                           "ks": bc.max_difference(flat(out["ks"]), t_ks), "energy": bc.max_difference(flat(out["energy"]), t_energy),
                           "terms": bc.max_difference(flat(out["terms"]), t_terms)},
            "fp64_row_pairs": int(sub.numel()),
            "hip_against_fp64": {k: bc.max_difference(flat(out[k])[sub].double(), want[k]) for k in want},
            "torch_ops_against_fp64": {k: bc.max_difference(torch32[k][sub].double(), want[k]) for k in want},
            "row_pairs_without_a_live_particle": int(torch.isnan(out["energy"]).sum()),
            "mean_wasserstein": [float(v) for v in out["wasserstein"].nan_to_num(0.0).mean((0, 1))],
            "mean_cramer": [float(v) for v in out["cramer"].nan_to_num(0.0).mean((0, 1))],
            "mean_ks": [float(v) for v in out["ks"].nan_to_num(0.0).mean((0, 1))],
            "mean_energy": float(out["energy"].nan_to_num(0.0).mean())}


def main():
    args = bc.arg_parser(__doc__).parse_args()
    dev = torch.device("cuda:0")
    cases = (("filtered_vs_marginal_smoothed", 32, 300, 300, 100), ("filtered_vs_marginal_smoothed", 32, 4096, 4096, 20),
             ("300_vs_4096_particles", 32, 300, 4096, 20))
    doc = {"device": torch.cuda.get_device_name(0), "cases": [case(*c, args.reps, dev) for c in cases]}
    bc.write_document(doc, args.out)


if __name__ == "__main__":
    main()
