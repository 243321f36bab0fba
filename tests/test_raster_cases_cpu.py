"""The belief-map rasteriser (``include/mmf.h``: ``MmfPfRasterArgs`` / ``mmf_pf_raster``) without a GPU: the reference's known
answers, the cap on the family of ``_raster_cases`` that makes the GPU bar fair, the entry point's host-side refusals, the
struct against the header as gcc lays it out, the ``ValueError``s of ``ParticleFilter.belief_maps`` on a CPU filter, and
``evaluation.map_axes`` / ``map_summary`` on a hand-made record."""
import ctypes
import inspect
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import _raster_cases as rc
import _smooth_cases as sc
import _summary_cases as sm
from _tol import REL_TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ETOOLARGE = -1, -2
_INPUTS = ("states", "log_a", "log_b", "center", "bandwidth")
_POINTERS = _INPUTS + ("density",)


# ------------------------------------------------------------------------------------------ 1. the definition, known answers
def _one(X, la, center, h, dims, cells, step):
    case = dict(states=np.asarray(X, np.float32), log_a=None if la is None else np.asarray(la, np.float32), log_b=None,
                center=np.asarray(center, np.float32), bandwidth=np.asarray(h, np.float32), dims=dims, cells=cells, step=step)
    return case, rc.reference(case)


def test_one_live_particle_gives_the_gaussian_product_in_closed_form():
    X = [[[0.25, -1.5, 0.75], [np.nan, np.nan, np.nan]]]
    case, ref = _one(X, [[0.0, -np.inf]], [[0.5, 0.5]], [[0.3, 0.7]], (2, 0), (5, 4), (0.25, 0.5))
    u, v = rc.axes(case["center"], case["step"], case["cells"])
    assert u.shape == (1, 5) and v.shape == (1, 4) and u[0, 2] == np.float32(0.5)      # odd count: the middle cell is the centre
    np.testing.assert_array_equal(u[0], np.float32([0.0, 0.25, 0.5, 0.75, 1.0]))
    np.testing.assert_array_equal(v[0], np.float32([-0.25, 0.25, 0.75, 1.25]))
    hx, hy = float(np.float32(0.3)), float(np.float32(0.7))
    for j in range(4):
        for i in range(5):
            want = (math.exp(-0.5 * ((float(u[0, i]) - 0.75) / hx) ** 2) * math.exp(-0.5 * ((float(v[0, j]) - 0.25) / hy) ** 2)
                    / (2.0 * math.pi * hx * hy))
            assert abs(ref[0, j, i] - want) <= 1e-14 * want, (j, i)


def test_the_mass_of_a_window_that_spans_six_bandwidths_around_every_particle_is_one():
    rng = np.random.default_rng(5)
    X = rng.uniform(-1.0, 1.0, (2, 40, 2)).astype(np.float32)
    la = rng.standard_normal((2, 40)).astype(np.float32)
    h = np.float32([[0.25, 0.5], [0.5, 0.25]])                         # h >= 2 steps
    cells, step = (64, 64), (0.125, 0.125)                             # the window: +- 4 around 0, particles within +- 1, 6 h = 3
    case, ref = _one(X, la, np.zeros((2, 2)), h, (0, 1), cells, step)
    mass = ref.sum((1, 2)) * step[0] * step[1]
    assert np.abs(mass - 1.0).max() < 1e-3, mass


def test_swapping_dims_and_cells_transposes_the_reference():
    case, ref = rc.family_case(65, 3, 3, "plain", (31, 33), (2, 0))
    swapped = dict(case, dims=(0, 2), cells=(33, 31), step=case["step"][::-1], center=case["center"][:, ::-1].copy(),
                   bandwidth=case["bandwidth"][:, ::-1].copy())
    # (the weight is multiplied into the y factor, so the two products round differently: fp64 ulps, not bits)
    np.testing.assert_allclose(rc.reference(swapped), ref.transpose(0, 2, 1), rtol=1e-13, atol=0.0)


def test_nan_rows_are_the_rows_of_the_definition_and_no_others():
    for variant in ("dead_row", "nan_center", "bad_bandwidth"):
        for cells in ((2, 2), (33, 31)):
            case, ref = rc.family_case(65, 3, 3, variant, cells, (0, 1))
            nan = np.isnan(ref).all((1, 2))
            assert nan.tolist() == [False, True, False] and not np.isnan(ref[~nan]).any(), variant
            assert rc.nan_rows(case).tolist() == nan.tolist()
    kinds = set()  # and over the family every kind of bad bandwidth occurs
    for case_id in rc.family():
        if case_id[3] == "bad_bandwidth":
            h = rc.make_case(*case_id)["bandwidth"][case_id[2] // 2]
            kinds |= {"nan" if math.isnan(b) else b for b in h.tolist() if not (0 < b < math.inf)}
    assert kinds == {"nan", 0.0, -0.5, math.inf}


# ------------------------------------------------------------------------------------------ 2. the family is certified
@pytest.mark.parametrize("M", rc.ALL_MS)
def test_the_fp32_formulation_is_within_the_cap_on_the_family(M):
    """A condition on the INPUTS: where fp32 torch ops cannot hold ``CAP = REL_TOL / 3`` against fp64, the kernel could not
    be asked for ``REL_TOL`` either.  Every case is held to it, none is skipped; and the case conditions hold."""
    worst, cases = 0.0, 0
    for case_id in rc.family():
        if case_id[0] != M:
            continue
        case, ref = rc.family_case(*case_id)
        span = np.asarray(case["cells"]) * np.asarray(case["step"])
        h = case["bandwidth"]
        assert all(not (0 < b < math.inf) or b >= span[k] / 64 for row in h for k, b in enumerate(row)), case_id
        ok = ~rc.nan_rows(case)
        assert (ref[ok].max((1, 2)) >= 1e-30).all(), case_id
        err = rc.map_err(rc.torch_formulation(case).numpy(), ref, str(case_id))
        assert err < rc.CAP, (case_id, err)
        worst, cases = max(worst, err), cases + 1
    assert cases >= len(rc.VARIANTS)
    print(f"M={M}: fp32 formulation against fp64, worst over {cases} cases {worst:.2e} (cap {rc.CAP:.0e})")


def test_the_family_covers_what_the_definition_distinguishes():
    seen = set(rc.family())
    assert rc.CAP <= REL_TOL / 3
    assert {c[0] for c in seen} == set(rc.ALL_MS) >= {1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 4096}
    assert {rc.ONE_STAGE - 1, rc.ONE_STAGE + 1, rc.TWO_STAGES - 1, rc.TWO_STAGES, rc.TWO_STAGES + 1} <= set(rc.ALL_MS)
    for M in rc.ALL_MS:
        mine = [c for c in seen if c[0] == M]
        assert {c[3] for c in mine} == set(rc.VARIANTS)
        if M <= rc.SMALL:  # the whole cross
            assert len(mine) == len(rc.CELLS) * len(rc.DIMS) * len(rc.RS) * len(rc.VARIANTS)
            assert {c[4] for c in mine} == set(rc.CELLS) and {c[1] for c in mine} == {2, 3, 4} and {c[2] for c in mine} == {1, 3}
    for d, pairs in rc.DIMS.items():
        assert (d - 1, 0) in pairs and {c[5] for c in seen if c[1] == d} == set(pairs)
    assert any(p[0] > p[1] for p in rc.DIMS[2])  # a reversed pair
    case = rc.make_case(257, 3, 3, "plain")
    assert np.isnan(case["states"]).any() and np.isinf(case["log_b"]).any()  # kill_an_eighth: dead particles hold NaN states


# ------------------------------------------------------------------------------------------ 3. the entry point's host checks
def _args(alias=None, dims=(0, 1), cells=(4, 2), step=(0.5, 0.25), **over):
    """Sizes at which every array fits the 16-float buffer ``host_args`` gives it."""
    from multimodalfilter_amd import _abi

    a = sc.host_args(_abi.MmfPfRasterArgs, _POINTERS, **{**dict(R=2, M=2, d=2), **over})
    for k in range(2):
        a.dims[k], a.cells[k], a.step[k] = dims[k], cells[k], step[k]
    return sc.alias_host_args(a, _POINTERS, alias)


def test_raster_refuses_bad_arguments_on_the_host():
    """Every refusal of the header with its return code, decided before any HIP call: the pointers are host memory and never
    dereferenced, the stream is null, and no GPU is needed."""
    lib = sc.lib()
    assert lib.mmf_version() == 42
    call = lambda alias=None, **over: lib.mmf_pf_raster(ctypes.byref(_args(alias, **over)), None)
    assert lib.mmf_pf_raster(None, None) == EINVAL
    for name in ("states", "center", "bandwidth", "density"):
        assert call(**{name: None}) == EINVAL, name
    assert call(log_a=None, log_b=None, R=0) == 0
    assert call(d=1, dims=(0, 0)) == EINVAL and call(d=0) == EINVAL and call(d=5) == EINVAL and call(d=-1) == EINVAL
    assert call(d=4, dims=(3, 0), R=0) == 0 and call(d=3, dims=(2, 1), R=0) == 0
    for bad in ((0, 0), (1, 1), (-1, 0), (0, 2), (2, 0), (0, -1)):
        assert call(dims=bad) == EINVAL, bad
    for bad in ((1, 4), (4, 1), (0, 4), (4, 129), (129, 4), (-3, 4)):
        assert call(cells=bad) == EINVAL, bad
    assert call(cells=(128, 128), R=0) == 0 and call(cells=(2, 2), R=0) == 0
    for bad in (0.0, -1.0, math.nan, math.inf, -math.inf):
        assert call(step=(bad, 0.5)) == EINVAL and call(step=(0.5, bad)) == EINVAL, bad
    assert call(M=0) == EINVAL and call(M=-2) == EINVAL and call(R=-1) == EINVAL
    for target in _INPUTS:
        assert call({"density": (target, 0)}) == EINVAL, target
    assert call({"density": ("states", 28)}) == EINVAL and call({"density": ("center", 12)}) == EINVAL   # partly on top
    assert call(M=16385) == ETOOLARGE and call(M=1 << 20) == ETOOLARGE
    assert call(M=16385, states=None) == EINVAL                          # an invalid call is invalid whatever its size
    assert call(R=1 << 30, cells=(128, 128)) == ETOOLARGE                # R * blocks of a map beyond a 32-bit grid
    assert call(R=0) == 0 and call(R=0, M=16384, d=4) == 0 and call(R=0, M=16385) == ETOOLARGE
    assert call({"density": ("states", 0)}, R=0) == 0                    # no rows: the arrays are empty, nothing overlaps


def test_the_binding_refuses_cpu_tensors_and_names_the_kernels_sizes():
    import torch

    from multimodalfilter_amd import _abi

    x = torch.zeros((2, 4, 3))
    c, h, out = torch.zeros((2, 2)), torch.ones((2, 2)), torch.zeros((2, 4, 4))
    with pytest.raises(_abi.MmfError):
        _abi.pf_raster(x, None, None, c, h, out, dims=(0, 1), step=(0.1, 0.1))
    with pytest.raises(_abi.MmfError, match="two"):
        _abi.pf_raster(x, None, None, c, h, out, dims=(0, 1, 2), step=(0.1, 0.1))
    assert _abi.RASTER_MAX_M == 16384 == rc.MAX_M and _abi.RASTER_MAX_CELLS == rc.MAX_CELLS == 128
    assert (_abi.RASTER_WAVES, _abi.RASTER_STAGE) == (rc.WAVES, rc.STAGE)


def test_the_raster_struct_matches_the_header_as_gcc_lays_it_out(tmp_path):
    """``MmfPfRasterArgs`` of ``_abi.py`` against ``include/mmf.h`` compiled as plain C: ``sizeof`` and every ``offsetof``."""
    from multimodalfilter_amd import _abi

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmf.h")).read(), flags=re.S)
    assert re.search(r"^\}\s*MmfPfRasterArgs\s*;", text, re.M) and re.search(r"^int\s+mmf_pf_raster\s*\(", text, re.M)
    assert "mmf_pf_raster" in _abi.SIGNATURES and _abi.ABI_VERSION == 42
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    cls = _abi.MmfPfRasterArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(ROOT, "include", "mmf.h")}"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(MmfPfRasterArgs));']
    lines += [f'  printf("{field} %zu\\n", offsetof(MmfPfRasterArgs, {field}));' for field, _t in cls._fields_]
    lines += ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines))
    out = subprocess.run([gcc, "-std=c99", "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    got = dict(line.split() for line in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(cls)
    for field, _t in cls._fields_:
        assert int(got[field]) == getattr(cls, field).offset, field


# ------------------------------------------------------------------------------------------ 4. the Python refusals
def test_belief_maps_refusals_come_before_any_device_work():
    import torch

    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import _abi, base

    sig = inspect.signature(mmf.filters.ParticleFilter.belief_maps).parameters
    assert list(sig) == ["self", "center", "span", "dims", "cells", "of", "bandwidth", "min_bandwidth", "likelihoods", "observations"]
    assert sig["dims"].kind is inspect.Parameter.KEYWORD_ONLY and sig["dims"].default == (0, 1) and sig["cells"].default == 64
    assert sig["of"].default == "filtered" and sig["bandwidth"].default == "silverman" and sig["min_bandwidth"].default == 1e-6
    assert sig["likelihoods"].default is False and sig["observations"].default is None
    pf = mmf.door_models.DoorParticleFilter().eval()
    assert pf.last_maps is None
    for of in ("filtered", "predicted"):
        with pytest.raises(ValueError, match="^belief_maps needs a history"):
            pf.belief_maps(torch.zeros((4, 2, 3)), (1.0, 1.0), of=of)
    with pytest.raises(ValueError, match=r"^belief_maps\(of='smoothed'\) needs a smoothed record"):
        pf.belief_maps(torch.zeros((4, 2, 3)), (1.0, 1.0), of="smoothed")
    for bad in ("posterior", "prior", None, 0):
        with pytest.raises(ValueError, match="of must be 'predicted', 'filtered' or 'smoothed'"):
            pf.belief_maps(torch.zeros((4, 2, 3)), (1.0, 1.0), of=bad)

    made = sc.cpu_filter_with_history()
    f, (T, N, M, d) = made.f, made.dims
    c = torch.zeros((T, N, d))
    before = {k: v for k, v in vars(f).items() if k.startswith("last_")}
    f.last_smoothed = base.belief_record(indices=torch.zeros((T, N), dtype=torch.int32), log_posterior=torch.zeros(N), lag=None,
                                         method="map")
    with pytest.raises(ValueError, match="not a\\s+distribution"):
        f.belief_maps(c, (1.0, 1.0), of="smoothed")
    f.last_smoothed = before["last_smoothed"]
    for bad in ((0, 0), (0, 3), (-1, 0), (0,), (0, 1, 2), (0.0, 1), (True, 0), "01", None, 1):
        with pytest.raises(ValueError, match="dims must be two distinct state dimensions in 0 .. 2"):
            f.belief_maps(c, (1.0, 1.0), dims=bad)
    for bad in (1, 129, 0, -4, (64,), (64, 1), (129, 64), (64, 64, 64), 64.0, True, "64", None):
        with pytest.raises(ValueError, match="cells must be an int or \\(Gx, Gy\\), each in 2 .. 128"):
            f.belief_maps(c, (1.0, 1.0), cells=bad)
    for bad in ((), (1.0,), (1.0, 0.0), (-1.0, 1.0), (1.0, math.nan), (math.inf, 1.0), (1.0, 1.0, 1.0), 1.0, "11", None,
                (True, 1.0), (1e-60, 1.0)):
        with pytest.raises(ValueError, match="span must be two positive finite floats"):
            f.belief_maps(c, bad)
    for bad in (torch.zeros((T, N)), torch.zeros((T + 1, N, d)), torch.zeros((T, N, 2)), np.zeros((T, N, d)), None):
        with pytest.raises(ValueError, match="center must be a \\(T, N, d\\)"):
            f.belief_maps(bad, (1.0, 1.0))
    with pytest.raises(ValueError, match="bandwidth must be 'silverman', 'scott' or 3"):
        f.belief_maps(c, (1.0, 1.0), bandwidth=(1.0, 1.0))
    with pytest.raises(ValueError, match="min_bandwidth"):
        f.belief_maps(c, (1.0, 1.0), min_bandwidth=0.0)
    # likelihood maps: a measurement model that fuses nothing leaves no observations in the history
    with pytest.raises(ValueError, match="pass observations="):
        f.belief_maps(c, (1.0, 1.0), likelihoods=True)
    for bad in ({"z": torch.zeros((T, N + 1, d))}, {"z": torch.zeros((T,))}, {"z": np.zeros((T, N, d))}):
        with pytest.raises(ValueError, match="observations must lead with \\(T, N\\)"):
            f.belief_maps(c, (1.0, 1.0), likelihoods=True, observations=bad)
    big = base.history_record(states=torch.zeros((1, 1, rc.MAX_M + 1, 2)), log_likelihoods=torch.zeros((1, 1, rc.MAX_M + 1)),
                              log_weights_in=None, ancestors=None, resampled=None, controls=None)
    f.last_history = big
    with pytest.raises(ValueError, match="16384"):
        f.belief_maps(torch.zeros((1, 1, 2)), (1.0, 1.0))
    f.last_history = before["last_history"]
    f.train()
    with pytest.raises(RuntimeError, match="eval"):
        f.belief_maps(c, (1.0, 1.0))
    f.eval()
    after = {k: v for k, v in vars(f).items() if k.startswith("last_")}
    assert after.keys() == before.keys() and all(after[k] is before[k] for k in before) and f.last_maps is None
    # and with everything in order the call reaches the library, which refuses host memory: there is no torch fallback
    for kw in (dict(), dict(of="predicted", cells=(33, 31), dims=(2, 0)), dict(bandwidth=(0.5, 2.0, 1.0)),
               dict(likelihoods=True, observations={"z": torch.zeros((T, N, d))})):
        with pytest.raises(_abi.MmfError):
            f.belief_maps(c, (1.0, 2.0), **kw)
    assert f.last_maps is None


# ------------------------------------------------------------------------------------------ 5. evaluation.map_axes / map_summary
def test_map_axes_and_map_summary_on_a_hand_made_record():
    import torch

    from multimodalfilter_amd import base, evaluation

    T, N, Gx, Gy = 3, 1, 3, 2
    center = torch.tensor([[[1.0, -2.0]], [[0.5, 0.25]], [[0.0, 0.0]]])
    density = torch.zeros((T, N, Gy, Gx))
    density[0, 0, 1, 2] = 4.0                # the peak of step 0: cell (i = 2, j = 1)
    density[0, 0, 0, 0] = 4.0                # ... and a tie before it: the first maximum wins, cell (0, 0)
    density[1] = math.nan                    # a step without a live particle
    density[2, 0, 0, 1] = 1.0
    density[2, 0, 1, 1] = 3.0                # cell (1, 1)
    mass = torch.tensor([[0.5], [math.nan], [0.25]])
    rec = base.belief_record(density=density, mass=mass, center=center, step=(0.5, 0.25), dims=(2, 0), cells=(Gx, Gy),
                             span=(1.5, 0.5), bandwidth=torch.ones((T, N, 2)), of="filtered", rule="silverman")
    x, y = evaluation.map_axes(rec)
    assert x.shape == (T, N, Gx) and y.shape == (T, N, Gy) and x.dtype == y.dtype == torch.float32
    assert x[0, 0].tolist() == [0.5, 1.0, 1.5] and y[0, 0].tolist() == [-2.125, -1.875]
    assert x[1, 0, 1] == 0.5                                           # an odd count: the centre itself
    ux, vy = rc.axes(center.numpy().reshape(T, 2), rec.step, rec.cells)
    assert np.array_equal(x.numpy().reshape(T, Gx), ux) and np.array_equal(y.numpy().reshape(T, Gy), vy)
    got = evaluation.map_summary(rec, start=0)
    assert got == {"mass": 0.375}
    true = torch.zeros((T, N, 3))
    true[0, 0] = torch.tensor([-2.125, 9.0, 0.5 + 3.0])                # dims = (2, 0): x is state 2, y is state 0
    true[2, 0] = torch.tensor([0.125 + 4.0, 9.0, 0.0])
    got = evaluation.map_summary(rec, true, start=0)
    assert set(got) == {"mass", "peak_error"} and abs(got["peak_error"] - 3.5) < 1e-12   # (3 + 4) / 2: the NaN step is left out
    assert abs(evaluation.map_summary(rec, true, start=2)["peak_error"] - 4.0) < 1e-12
    assert inspect.signature(evaluation.map_summary).parameters["start"].default == evaluation.START_TRUNCATION
    # agreement: a likelihood map proportional to the density agrees fully, one on other cells not at all
    ll = torch.full((T, N, 2, Gy, Gx), -math.inf)
    ll[0, 0, 0] = torch.log(density[0, 0]) + 7.0
    ll[0, 0, 1, 0, 1] = 0.0
    ll[2, 0, 0] = torch.log(density[2, 0]) - 3.0
    ll[2, 0, 1] = 0.0                                                  # flat: sqrt(p / 6) summed
    ll[1] = 0.0
    rec.log_likelihood = ll
    got = evaluation.map_summary(rec, start=0)["agreement"]
    flat = (math.sqrt(0.25 / 6) + math.sqrt(0.75 / 6))
    assert got.shape == (2,) and got.dtype == torch.float32
    assert abs(float(got[0]) - 1.0) < 1e-6 and abs(float(got[1]) - 0.5 * flat) < 1e-6
    for bad in (base.belief_record(mass=mass), base.belief_record(density=density)):
        with pytest.raises(ValueError, match="belief_maps"):
            evaluation.map_summary(bad)
    with pytest.raises(ValueError, match="belief_maps"):
        evaluation.map_axes(base.belief_record(density=density))
    with pytest.raises(ValueError, match="true must be"):
        evaluation.map_summary(rec, torch.zeros((T, N, 2)), start=0)
