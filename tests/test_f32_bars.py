"""The bars of tests/f32_bars.py, computed on the CPU for every case the float32 GPU tests run: the float64 and
float32 oracles are finite there, no block's reference vanishes (a relative error would mean nothing), and no bar is
looser on a block than the whole-vector bars the suite had before (gradient 1e-4, E 2e-5); the second-order bars
stay ten times under the former 1e-3.

Measured on the CPU that wrote this (maximum over problems and the five point orders): the float32 oracle's worst
per-block gradient error is 6.6e-6 ((2, 130) ray angle, points, at the trial point), its worst E error 2.8e-6
((2, 5)), its worst slope error 2.4e-6, its worst H v block 1.14e-5 ((2, 130) ray angle, intrinsics), dE/dobs
4.7e-6 and the observation second-order output 4.7e-6, so the caps leave room for MARGIN.
"""
import pytest
import torch

import f32_bars

G_CAP, E_CAP, SECOND_CAP = 1e-4, 2e-5, 1e-4


def _check(reference, caps):
    assert reference.finite, reference.name
    for key, norm in f32_bars.reference_norms(reference).items():
        assert (norm > 0).all(), (reference.name, key, norm)
    for key, bar in reference.bar.items():
        assert torch.isfinite(bar).all() and (bar >= f32_bars.MARGIN * f32_bars.FLOOR).all(), (reference.name, key)
        cap = caps(key)
        if cap is not None:
            assert (bar <= cap).all(), (reference.name, key, bar.tolist(), cap)
    print("BARS", reference.name, {k: float(v.max()) for k, v in reference.bar.items()})


def _eval_caps(key):
    return E_CAP if key == "E" else G_CAP if key.startswith("grad.") else None  # (the slope has no former bar)


@pytest.mark.parametrize("trial", [False, True])
@pytest.mark.parametrize("name", list(f32_bars.CASES) + list(f32_bars.TAYLOR) + list(f32_bars.UNSEEN))
def test_evaluation_bars(name, trial):
    ref = f32_bars.evaluation_reference(name, trial)
    _check(ref, _eval_caps)
    if f32_bars.SCENES[name]["unseen"]:
        # the oracle gives view 1's rotation gradient as exactly zero; its translation and the unseen point keep the
        # scale path's rounding residue
        assert (ref.ref["grad"][:, f32_bars.rotation_entries(name, 1)] == 0.0).all()
        zeros = ref.ref["grad"][:, f32_bars.zero_entries(name)].abs().max(dim=-1).values
        assert (zeros <= 1e-15 * ref.ref["grad"].norm(dim=-1)).all(), zeros
    if f32_bars.SCENES[name]["taylor"] is not None:
        x = f32_bars.trial_point(name) if trial else f32_bars.scene(name)[0]
        assert (x[:, f32_bars.rotation_entries(name, 1)] == 0.0).all()
        assert torch.equal(x[:, f32_bars.rotation_entries(name, 2)],
                           f32_bars.scene(name)[0][:, f32_bars.rotation_entries(name, 2)])


@pytest.mark.parametrize("which", f32_bars.WHICH)
@pytest.mark.parametrize("name", list(f32_bars.SECOND))
def test_second_order_bars(name, which):
    ref = f32_bars.second_reference(name, which)
    assert not ref.undefined.any() and not ref.undefined32.any()
    _check(ref, lambda key: SECOND_CAP)


@pytest.mark.parametrize("name", list(f32_bars.TAYLOR))
def test_second_order_bars_on_the_taylor_branches(name):
    """A rotation that is exactly zero: torch's double backward of |w| at w = 0 leaves H v undefined on view 1's
    three rotation entries, in both precisions, and nowhere else."""
    ref = f32_bars.second_reference(name, "both")
    expected = torch.zeros_like(ref.undefined)
    expected[:, f32_bars.rotation_entries(name, 1)] = True
    assert torch.equal(ref.undefined, expected) and torch.equal(ref.undefined32, expected)
    _check(ref, lambda key: SECOND_CAP)


def test_blocks_tile_the_parameter_vector():
    for m, n, distortion in ((2, 1, False), (3, 70, True), (5, 63, False)):
        covered = []
        for cols in f32_bars.blocks(m, n, distortion).values():
            covered += list(range(cols.start, cols.stop))
        assert covered == list(range(3 + 3 * n + 6 * (m - 1) + (5 if distortion else 0)))
