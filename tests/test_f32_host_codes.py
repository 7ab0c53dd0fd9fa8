"""What the float32 fused host entry points return, held to a recording (tests/golden/f32_host_codes.json, written by
tests/golden/make_f32_host_codes.py from the build before each operation's launch plan was gathered into one
derivation): the adjoint's and the gradient descent's size queries over the solve plan table's grid, the view-count
edges and the overrides that table does not cross, and the seven launch entry points on arguments the host refuses
-- the codes and, in the rows with two defects, their precedence.  No GPU: the queries are pure, and every launch
row returns before a device is touched."""
import importlib.util
import json
import os

import pytest
import torch

from conftest import GOLDEN


def _load_generator():
    spec = importlib.util.spec_from_file_location("make_f32_host_codes",
                                                  os.path.join(GOLDEN, "make_f32_host_codes.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


gen = _load_generator()


@pytest.fixture(scope="module")
def recorded():
    with open(gen.OUT) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def native():
    from deep_attention_visual_odometry_amd import _native

    yield _native.load_library(), _native
    _native.clear_debug_overrides()


@pytest.fixture(scope="module")
def launch_rows(native, recorded):
    """The recorded launch rows, rebuilt from this build's queries: the same rows, or none is run."""
    rows, expect = gen.candidate_rows(*native), "".join(recorded["launch_expect"])
    assert gen.rows_digest(rows) == recorded["launch_rows_sha256"], "not the recorded rows: a query differs"
    assert len(rows) == len(expect) == 1744  # no row dropped
    return [dict(r, expect=int(e)) for r, e in zip(rows, expect)]


def test_every_query_returns_the_recorded_integers(native, recorded):
    lib, N = native
    rows = list(gen.query_rows())
    assert len(gen.SHAPES) == 27 and len(gen.OVERRIDES) == 10
    assert len(rows) == len(recorded["query_rows"]) == 27 * 3 * 2 * 2 * 13 * 10  # the whole grid
    wrong = {}
    for (key, spec), index in zip(rows, recorded["query_rows"]):
        got, want = gen.run_query(lib, N, spec), recorded["query_values"][index]
        if got != want:
            wrong[key] = (got, want)
    assert not wrong, f"{len(wrong)} query rows differ, e.g. {sorted(wrong.items())[:5]} ({recorded['query_symbols']})"


def test_the_recorded_launch_rows_cover_every_symbol_and_cannot_launch(launch_rows):
    assert {r["sym"] for r in launch_rows} == set(gen.LAUNCH_SYMBOLS) and len(gen.LAUNCH_SYMBOLS) == 7
    assert len({r["id"] for r in launch_rows}) == len(launch_rows)
    for r in launch_rows:
        assert r["expect"] in ((0, 1, 2, 4) if gen.may_return_ok(r) else (1, 2, 4)), r["id"]


@pytest.mark.skipif(torch.cuda.is_available(),
                    reason="host logic: a refusal that regressed into an acceptance would launch on null pointers")
def test_every_refused_launch_returns_the_recorded_status(native, launch_rows):
    lib, N = native
    wrong = {}
    for r in launch_rows:
        got = int(gen.run_launch(lib, N, r))
        if got != r["expect"]:
            wrong[r["id"]] = (got, r["expect"])
    assert not wrong, f"{len(wrong)} of {len(launch_rows)} launch rows differ: {sorted(wrong.items())[:10]}"
