"""Regularised resampling (``include/mmf.h``: ``mmf_pf_regularise``): the definition restated in numpy, the case set of the
GPU test, and the gcc twin of the counter-based normals.

``reference`` evaluates the definition in the dtype it is given: float64 is the reference the kernel is held to, float32
the restatement that shows the case set to be feasible (``tests/test_regularise_cases_cpu.py``).

The case recipe: ``C = A A^T`` with ``A = s (I + 0.3 G)`` redrawn until ``cond(C) <= 100``, ``s`` cycling through
``{1e-2, 0.3, 1, 30}``, ``ess`` uniform in ``[1, M]``; the sets are CENTRED -- ``|mu|`` of the order of the spread -- because
a displacement ``x' - x`` of a set far from the origin is not recoverable from fp32 outputs to 1e-4 (rounding alone leaves
4e-5 .. 9e-5 there); ``factor`` and ``bandwidth`` are held separately instead of differencing outputs.  Special rows, in
every batch: a rank-deficient ``C`` (the last direction has zero variance), ``C = 0``, a NaN ``C``, a NaN ``ess`` and a row
that an ESS-triggered step kept (``resampled == 0``)."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N = 12
SHAPES = [(M, d) for M in (30, 300, 1025) for d in (1, 2, 3, 4)]
FLOORS = (0.0, 0.05)
SCALES_OF_ROWS = (1e-2, 0.3, 1.0, 30.0)
ROW_RANK, ROW_ZERO, ROW_NAN_COV, ROW_NAN_ESS, ROW_KEPT = 7, 8, 9, 10, 11  # rows 0 .. 6 are regular
UNCHANGED_ROWS = (ROW_NAN_COV, ROW_NAN_ESS, ROW_KEPT)
SCALE = 1.0


def silverman(ess, d, scale, dtype=np.float64):
    ess = np.asarray(ess, dtype=dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        return dtype(scale) * np.power(dtype(4.0) / (dtype(d + 2) * ess), dtype(1.0) / dtype(d + 4))


def clamped_cholesky(C, floor, dtype=np.float64):
    """The definition's factor of ``C + diag(floor^2)`` for one ``(d, d)`` matrix: a non-positive (or NaN) pivot gives a zero
    column."""
    C = np.asarray(C, dtype=dtype)
    d = C.shape[0]
    f2 = np.asarray(floor, dtype=dtype) ** 2
    L = np.zeros((d, d), dtype=dtype)
    for j in range(d):
        s = C[j, j] + f2[j] - np.sum(L[j, :j] * L[j, :j], dtype=dtype)
        L[j, j] = np.sqrt(s) if s > 0 else 0
        for i in range(j + 1, d):
            L[i, j] = (C[i, j] - np.sum(L[i, :j] * L[j, :j], dtype=dtype)) / L[j, j] if L[j, j] > 0 else 0
    return L


def reference(x, mu, C, ess, eps, *, scale, floor, shrink, resampled=None, dtype=np.float64):
    """``(x', factor, bandwidth)`` of the definition, in ``dtype``.  A row that is left unchanged is returned as it came (the
    same array values), its factor is zero; ``bandwidth`` is NaN where ``ess`` is not finite or ``< 1`` and 0 where
    ``resampled == 0``."""
    x, mu, C, ess, eps = (np.asarray(a, dtype=dtype) for a in (x, mu, C, ess, eps))
    n_traj, M, d = x.shape
    floor = np.broadcast_to(np.asarray(floor, dtype=dtype), (d,))
    out = x.copy()
    factor = np.zeros((n_traj, d, d), dtype=dtype)
    bandwidth = np.full((n_traj,), np.nan, dtype=dtype)
    for n in range(n_traj):
        kept = resampled is not None and int(resampled[n]) == 0
        ess_ok = bool(np.isfinite(ess[n]) and ess[n] >= 1)
        h = silverman(ess[n], d, scale, dtype) if ess_ok else dtype(np.nan)
        bandwidth[n] = 0 if kept else h
        if kept or not ess_ok or not np.all(np.isfinite(C[n])):
            continue
        H = (h * clamped_cholesky(C[n], floor, dtype)).astype(dtype)
        factor[n] = H
        base = x[n]
        if shrink:
            a = np.sqrt(np.maximum(dtype(1) - h * h, dtype(0)))
            base = mu[n] + a * (x[n] - mu[n])
        out[n] = base + eps[n] @ H.T
    return out, factor, bandwidth


def make_case(M, d, seed=0):
    """float32 inputs of one batch: ``x (N, M, d)``, ``mu (N, d)``, ``C (N, d, d)``, ``ess (N)``, ``eps (N, M, d)``,
    ``resampled (N)`` int32.  ``mu`` and ``C`` are the set's own (uniform-weight) moments, as K1 would report them, up to
    rounding; the special rows are built to the letter (exact zeros, exact constants)."""
    rng = np.random.default_rng(1000 * M + 10 * d + seed)
    x = np.zeros((N, M, d))
    mu = np.zeros((N, d))
    C = np.zeros((N, d, d))
    for n in range(N):
        s = SCALES_OF_ROWS[n % len(SCALES_OF_ROWS)]
        while True:
            A = s * (np.eye(d) + 0.3 * rng.standard_normal((d, d)))
            C[n] = A @ A.T
            if np.linalg.cond(C[n]) <= 100.0:
                break
        mu[n] = s * rng.standard_normal(d)
        x[n] = mu[n] + rng.standard_normal((M, d)) @ A.T
    ess = rng.uniform(1.0, M, size=N)
    ess[0], ess[1] = 1.0, float(M)  # both ends of K1's range
    # the special rows
    if d > 1:  # the last direction has no variance: its row and column of C are exact zeros, the coordinate is a constant
        C[ROW_RANK, -1, :] = 0.0
        C[ROW_RANK, :, -1] = 0.0
        x[ROW_RANK, :, -1] = mu[ROW_RANK, -1]
    else:
        C[ROW_RANK] = 0.0
        x[ROW_RANK] = mu[ROW_RANK]
    C[ROW_ZERO] = 0.0
    x[ROW_ZERO] = mu[ROW_ZERO]
    C[ROW_NAN_COV, 0, 0] = np.nan
    ess[ROW_NAN_ESS] = np.nan
    resampled = np.ones((N,), dtype=np.int32)
    resampled[ROW_KEPT] = 0
    eps = rng.standard_normal((N, M, d))
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    x, mu = f32(x), f32(mu)
    for n in (ROW_RANK, ROW_ZERO):  # (the constants after rounding to float32)
        cols = slice(None) if n == ROW_ZERO or d == 1 else slice(d - 1, d)
        x[n][:, cols] = mu[n][cols]
    return dict(x=x, mu=mu, C=f32(C), ess=f32(ess), eps=f32(eps), resampled=resampled)


def rel_err_rows(got, want, dims=None):
    """``_tol.rel_err`` trajectory by trajectory over the rows whose reference is finite -- the worst vector of a row against
    that ROW's scale, so that a row of scale 1e-2 is not measured against the batch's scale 30 -- and the worst row."""
    from _tol import rel_err

    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    worst = 0.0
    for n in range(want.shape[0]):
        if np.all(np.isfinite(want[n])):
            worst = max(worst, rel_err(got[n], want[n], dims=dims))
    return worst


def build_philox(tmp_path) -> str:
    """Compile ``tests/regularise_philox.c`` against ``include/mmf_philox.h`` with gcc into ``tmp_path``."""
    exe = os.path.join(str(tmp_path), "regularise_philox")
    cmd = ["gcc", "-O2", "-ffp-contract=off", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", exe,
           os.path.join(ROOT, "tests", "regularise_philox.c"), "-lm"]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return exe


def philox_normals(exe, seed, stream, step, traj0, n_traj, M):
    """``(z (n_traj, M, 4) float32, legacy_equal)`` from the gcc program: the four normals of every particle on ``stream``, and
    whether ``mmf_philox_normal4`` equalled stream 0 bit for bit on the same counters."""
    out = subprocess.run([exe, str(seed), str(stream), str(step), str(traj0), str(n_traj), str(M)], capture_output=True,
                         text=True, check=True).stdout.split("\n")
    words = np.array([[int(w, 16) for w in line.split()] for line in out[:n_traj * M]], dtype=np.uint32)
    assert out[n_traj * M].startswith("legacy_equal ")
    return words.view(np.float32).reshape(n_traj, M, 4), out[n_traj * M].split()[1] == "1"
