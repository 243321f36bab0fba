"""The feature benchmarks ``scripts/bench_*.py`` and what they share (``scripts/_bench_common.py``), as far as a host without a
device can tell: every script loads, and the helpers that touch no device do what they say."""
import glob
import importlib.util
import json
import os

import pytest

SCRIPTS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts")
BENCHMARKS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(SCRIPTS, "bench_*.py")))


@pytest.fixture
def bc(monkeypatch):
    monkeypatch.syspath_prepend(SCRIPTS)
    import _bench_common

    return _bench_common


def test_there_are_benchmarks_to_load():
    assert len(BENCHMARKS) >= 23 and "bench_maps.py" in BENCHMARKS


@pytest.mark.parametrize("name", BENCHMARKS)
def test_a_benchmark_loads_without_a_device(name, bc):
    import torch

    spec = importlib.util.spec_from_file_location("_loaded_" + name[:-3], os.path.join(SCRIPTS, name))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    assert callable(module.main)
    assert not torch.cuda.is_initialized()


def test_stats(bc):
    assert bc.stats([3.0, 1.0, 2.0]) == {"median": 2.0, "min": 1.0, "max": 3.0}


def test_write_document_writes_what_it_prints(bc, tmp_path, capsys):
    doc = {"device": "none", "cases": [{"batch": 2, "ms_per_call": {"a": bc.stats([1.5, 0.5])}, "span": [0.25, None]}]}
    out = tmp_path / "not" / "there" / "yet" / "doc.json"
    bc.write_document(doc, str(out))
    printed = capsys.readouterr().out
    assert out.read_text() == printed == json.dumps(doc, indent=1) + "\n"
    assert json.loads(printed) == doc
    bc.write_document(doc, None)
    assert capsys.readouterr().out == printed and sorted(os.listdir(tmp_path)) == ["not"]


def test_arg_parser_defaults(bc):
    args = bc.arg_parser("what is timed").parse_args([])
    assert args.reps == 7 and args.out is None
    args = bc.arg_parser("what is timed").parse_args(["--reps", "2", "--out", "x.json"])
    assert args.reps == 2 and args.out == "x.json"
