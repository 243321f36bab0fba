"""What the per-modality attribution costs (profiles/modalities/README.md): ``belief_modalities()`` on the history of the door
crossmodal particle filter at 32 x 300 x T = 100 and 32 x 4096 x T = 20, and its parts on the same tensors -- the observation
encoders over the ``T N`` rows (``encode_observations``), the re-evaluation of both measurement networks on the recorded
particles in one launch (``mmf_pf_measure_multi``), ``mmf_pf_modalities`` alone -- beside the formulation a caller would write
today in fp32 torch ops on the same device (``tests/_modality_cases.torch_rows``: logsumexps over ``(K + 1, R, M)`` arrays and
two ``einsum``s).  Device time from HIP events around each call, after a warm-up call of each, median / min / max of ``--reps``
calls, the runs alternating.

    python scripts/bench_modalities.py [--reps 7] [--out FILE]

One JSON document.  ``bytes``: ``4 (1 + K + d) R M``, what the summary has to read once; ``hip_bytes_per_second`` is that over
the kernel's median time, ``share_of_hbm`` that over the 6.3e12 B/s a streaming kernel achieves on an MI355X (8e12 peak).
``hip_modalities_x16`` is 16 launches between one pair of events, ``..._back_to_back`` the rate from a sixteenth of it; at both
sizes the inputs fit the 256 MiB Infinity Cache, so repeated calls measure the chip's caches, not HBM.  ``agreement``: the
largest difference between the two formulations' outputs (``log_evidence`` and ``divergence`` absolute, the others relative
to the largest entry)."""
import os
import statistics
import sys

import torch

import _bench_common as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_ACHIEVABLE = 6.3e12
HBM_PEAK = 8.0e12
BACK_TO_BACK = 16   # launches of the kernel between one pair of events: its time without the gap around a single launch


def case(N, M, T, reps, dev):
    import _modality_cases as mc
    from multimodalfilter_amd import _abi, engine, evaluation

    door = bc.recorded_door_run(N, M, T, dev)
    f, h, obs, d = door.f, door.f.last_history, door.obs, door.dims[3]
    R = T * N
    meas = f.measurement_model
    flat_obs = {k: v.reshape((R,) + tuple(v.shape[2:])) for k, v in obs.items()}
    with torch.no_grad():
        ctx = meas.encode_observations(flat_obs)
        nets, _ = meas.fused_measurements(ctx)
        logliks, beta, enabled = meas.modality_log_likelihoods(h.states.view(R, M, d), ctx)
    K = len(logliks)
    blobs, biases = [n.blob() for n, _, _ in nets], [b for _, b, _ in nets]
    n_res, prec = nets[0][0].n_res, nets[0][0].precision_code()
    states = h.states.view(R, M, d)
    scratch = [torch.empty_like(l) for l in logliks]
    f32 = lambda *s: torch.empty((T, N) + s, dtype=torch.float32, device=dev)
    out = dict(log_evidence=f32(K + 1), responsibility=f32(K), ess=f32(K + 1), mean=f32(K + 1, d), divergence=f32(K), overlap=f32(K, K))
    cols = [l.view(T, N, M) for l in logliks]
    beta_v = None if beta is None else beta.view(T, N, K)
    stacked = torch.stack(logliks)

    runs = {"belief_modalities": f.belief_modalities,                 # encoders + both networks + the summary + the record
            "encode_observations": lambda: meas.encode_observations(flat_obs),
            "measure_multi": lambda: _abi.pf_measure_multi(blobs, n_res, prec, states, biases, [None] * K, 0, scratch,
                                                           engine.range_flag(dev)),
            "hip_modalities": lambda: _abi.pf_modalities(h.states, h.log_weights_in, cols, beta_v, **out),
            "hip_modalities_x16": lambda: [_abi.pf_modalities(h.states, h.log_weights_in, cols, beta_v, **out) for _ in range(BACK_TO_BACK)],
            "torch_ops": lambda: mc.torch_rows(states, h.log_weights_in.view(R, M), stacked, beta)}
    with torch.no_grad():
        times = bc.time_alternating(runs, reps)
        runs["hip_modalities"]()
        ref = runs["torch_ops"]()
        torch.cuda.synchronize()
    med = {k: statistics.median(x) for k, x in times.items()}
    agreement = {}
    for k, got in out.items():
        want = ref[k].reshape(got.shape)
        ok = torch.isfinite(want) & torch.isfinite(got)
        diff = float((got - want)[ok].abs().max())
        agreement[k] = diff if k in ("log_evidence", "divergence") else diff / float(want[ok].abs().max())
        assert bool((torch.isnan(got) == torch.isnan(want)).all()), k
    for i, l in enumerate(logliks):
        assert torch.equal(scratch[i], l), "measure_multi is deterministic"
    byts = 4.0 * (1 + K + d) * R * M
    rate = byts / (1e-3 * med["hip_modalities"])
    rate_b2b = byts * BACK_TO_BACK / (1e-3 * med["hip_modalities_x16"])
    summary = evaluation.modality_summary(f.last_modalities, start=0)
    return {"filter": "DoorCrossmodalParticleFilter", "batch": N, "particles": M, "steps": T, "state_dim": d, "modalities": K,
            "rows": R, "workgroups": R, "threads": min(512, ((M + 3) // 4 + 63) // 64 * 64), "bytes": byts,
            "ms_per_call": {k: bc.stats(x) for k, x in times.items()},
            "torch_over_hip": med["torch_ops"] / med["hip_modalities"],
            "hip_bytes_per_second": rate, "share_of_hbm": rate / HBM_ACHIEVABLE, "share_of_hbm_peak": rate / HBM_PEAK,
            "hip_bytes_per_second_back_to_back": rate_b2b, "share_of_hbm_back_to_back": rate_b2b / HBM_ACHIEVABLE,
            "inputs_fit_the_infinity_cache": byts < 256 * 2 ** 20,
            "torch_bytes_per_second": byts / (1e-3 * med["torch_ops"]),
            "agreement": agreement,
            "summary": {k: v.tolist() for k, v in summary.items()}}


def main():
    args = bc.arg_parser(__doc__).parse_args()
    dev = torch.device("cuda:0")
    doc = {"device": torch.cuda.get_device_name(0),
           "cases": [case(N, M, T, args.reps, dev) for N, M, T in ((32, 300, 100), (32, 4096, 20))]}
    bc.write_document(doc, args.out)


if __name__ == "__main__":
    main()
