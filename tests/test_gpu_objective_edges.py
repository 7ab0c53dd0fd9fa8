"""The float32 evaluator (dava_ba_evaluate) and dual-number kernel (dava_ba_second_order) at edge shapes, in every
form and flavour, held per block of the parameter vector to bars derived from the oracle alone (tests/f32_bars.py:
reference, norms and the bar rule; tests/test_f32_bars.py checks the bars themselves on the CPU).

Each launch is compared with the float64 oracle at its own evaluation point -- x, or the float32 x + alpha d --
never with another launch.  B = 4, alpha = (0, 0.5, 1, 2): problem 0 is a trial point that is x itself.

Matrix cases (M, N, model): (2, 1) one point, 255 idle threads; (2, 5) fewer points than a wave; (5, 63) one short
of a wave, four moving views; (3, 70) Brown-Conrady, P = 230 is no multiple of 4; (2, 130) ray angle, one focal
slot on elu's exponential branch; (2, 260) the per-thread point loop runs twice for four threads; (2, 520)
Brown-Conrady, under FORCE_GV 8 threads hold a packed pair and the rest one scalar point; (3, 1030) global
vectors by itself, threads 0-5 hold a pair plus a scalar tail; (2, 1030) ray angle, where the packed sweep must not
apply.  Forms: the default one (asserted through the solve's plan), NO_PPT (N <= 256), FORCE_GV (vectors in LDS),
FORCE_GV + GV_NO_XL (vectors in place in HBM).

Measured on the MI355X: profiles/f32_eval_parity.jsonl (rewritten by a complete run with DAVA_WRITE_PROFILES=1).
"""
import pytest
import torch

import f32_bars

pytestmark = pytest.mark.gpu


def _launch(device, name, flavour, x=None):
    """One dava_ba_evaluate launch of a (gradient, slope, trial) flavour; CPU tensors (None where not produced)."""
    from deep_attention_visual_odometry_amd import native_ops

    c = f32_bars.SCENES[name]
    grad, slope, trial = (ch == "1" for ch in flavour)
    x0, obs, vis = f32_bars.scene(name)
    x0 = x0 if x is None else x
    d = f32_bars.direction(name).to(device) if (slope or trial) else None
    out = native_ops.ba_evaluate(x0.to(device), obs.to(device), vis.to(device), c["m"], c["n"], c["model"] == "bc",
                                 direction=d, alpha=f32_bars.alpha().to(device) if trial else None, want_grad=grad,
                                 want_slope=slope, residual=f32_bars.residual_of(name))
    assert (out[1] is not None) == grad and (out[2] is not None) == slope
    return tuple(None if t is None else t.cpu() for t in out)


def _set_form(overrides, form):
    for knob, value in f32_bars.FORM_OVERRIDES[form].items():
        overrides(knob, value)


def _sweep(device, name, tally, form):
    """All eight flavours of one scene in the form that is set, each against the oracle at its own point."""
    outs = {}
    for flavour in f32_bars.FLAVOURS:
        e, g, sl = outs[flavour] = _launch(device, name, flavour)
        reference = f32_bars.evaluation_reference(name, flavour[2] == "1")
        tally.add(f"{form}:{flavour}", reference, f32_bars.measure_evaluation(reference, e, g, sl))
    return outs


def _plan(name):
    from deep_attention_visual_odometry_amd import native_ops
    from deep_attention_visual_odometry_amd._native import DAVA_HESSIAN_DENSE

    c = f32_bars.SCENES[name]
    return native_ops.solve_plan(f32_bars.B, c["m"], c["n"], c["model"] == "bc", DAVA_HESSIAN_DENSE, 1,
                                 f32_bars.residual_of(name))


# ---- 1. the evaluator matrix ----

@pytest.mark.parametrize("name", list(f32_bars.CASES))
def test_default_form_is_the_one_the_case_is_meant_for(device, name):
    """plan_eval takes global-vector mode exactly where the solve's plan of a dense one-iteration config does (the
    same image against the same budget); with N <= 256 (a point per thread) that names the form, so a later change
    of a budget cannot silently move a case to another kernel."""
    gv = _plan(name)["global_vectors"] == 1
    form = "gv" if gv else "ppt" if f32_bars.SCENES[name]["n"] <= 256 else "lds"
    assert form == f32_bars.CASES[name]["default"]


@pytest.mark.parametrize("name,form", [(name, form) for name in f32_bars.CASES for form in f32_bars.forms_of(name)])
def test_every_flavour_matches_the_oracle_per_block(device, overrides, name, form):
    _set_form(overrides, form)
    assert form not in ("gv_xl", "gv_hbm") or _plan(name)["global_vectors"] == 1
    tally = f32_bars.Tally("eval", f"{name}/{form}")
    _sweep(device, name, tally, form)
    failures = tally.emit()
    assert not failures, failures


# ---- 2. Taylor branches ----

@pytest.mark.parametrize("form", f32_bars.TAYLOR_FORMS)
@pytest.mark.parametrize("name", list(f32_bars.TAYLOR))
def test_taylor_branches(device, overrides, name, form):
    """(3, 70) with view 1's rotation exactly zero (1 / theta taken as 0, every series at 0) and view 2's of norm
    1e-3 (both series) or 0.03 (the closed form of sin x / x, the series of (1 - cos x) / x^2 and of the slope of
    sinc).  The direction is zero on those six entries, so every flavour sees exactly these rotations."""
    _set_form(overrides, form)
    tally = f32_bars.Tally("taylor", f"{name}/{form}")
    _sweep(device, name, tally, form)
    failures = tally.emit()
    assert not failures, failures


# ---- 3. a view that sees nothing, a point nobody sees ----

@pytest.mark.parametrize("name", list(f32_bars.UNSEEN))
def test_nothing_seen(device, name):
    """vis[:, 1, :] and vis[:, :, 69] are False.  The oracle gives view 1's rotation gradient as exactly zero and
    view 1's translation and point 69 as the scale path's rounding residue: those nine entries are held to
    |g_i| <= FLOOR ||g_ref||, the pooled blocks to their bars, and everything must be finite."""
    tally = f32_bars.Tally("unseen", name)
    outs = _sweep(device, name, tally, "default")
    zeros, rot1 = f32_bars.zero_entries(name), f32_bars.rotation_entries(name, 1)
    worst, exact = 0.0, True
    for flavour, (e, g, sl) in outs.items():
        assert all(torch.isfinite(t).all() for t in (e, g, sl) if t is not None), flavour
        if g is None:
            continue
        reference = f32_bars.evaluation_reference(name, flavour[2] == "1")
        rel = g[:, zeros].double().abs().max(dim=-1).values / reference.ref["grad"].norm(dim=-1)
        worst = max(worst, float(rel.max()))
        exact = exact and bool((g[:, rot1] == 0.0).all())
    zero32 = max(float(f32_bars.evaluation_reference(name, t).zero32.max()) for t in (False, True))
    failures = tally.emit(zero_entries={"gpu": worst, "ref32": zero32, "bar": f32_bars.FLOOR},
                          view1_rotation_exactly_zero=exact)
    assert not failures, failures
    assert worst <= f32_bars.FLOOR, worst


# ---- 4. independence ----

def test_a_nan_problem_leaves_the_others_bitwise(device):
    name = "m3_n70_bc"
    x = f32_bars.scene(name)[0].clone()
    x[1] = float("nan")
    for flavour in ("111", "100"):
        clean, dirty = _launch(device, name, flavour), _launch(device, name, flavour, x=x)
        for s, t in zip(clean, dirty):
            if s is not None:
                assert torch.equal(s[[0, 2, 3]], t[[0, 2, 3]]) and torch.isfinite(s).all()


# ---- 5. the dual-number kernel ----

def _second(device, name, which):
    from deep_attention_visual_odometry_amd import native_ops

    c = f32_bars.SCENES[name]
    x, obs, vis = f32_bars.scene(name)
    v, u = f32_bars.second_directions(name, which)
    assert native_ops.second_order_form(f32_bars.B, c["m"], c["n"], c["model"] == "bc", f32_bars.residual_of(name)) == 0
    out = native_ops.ba_second_order(x.to(device), obs.to(device), vis.to(device), c["m"], c["n"], c["model"] == "bc",
                                     direction=None if v is None else v.to(device),
                                     residual=f32_bars.residual_of(name),
                                     obs_direction=None if u is None else u.to(device))
    return tuple(t.cpu() for t in out)


@pytest.mark.parametrize("which", f32_bars.WHICH)
@pytest.mark.parametrize("name", list(f32_bars.SECOND))
def test_second_order_matches_double_backward_per_block(device, name, which):
    """dava_ba_second_order (form 0; test_gpu_large_second.py shows forms 1 and 2 bitwise equal to it): dE/dx and
    H v + (d2E/dx dobs) u per block, dE/dobs and the observation second-order output per problem, against the
    float64 double backward through the oracle."""
    reference = f32_bars.second_reference(name, which)
    out = _second(device, name, which)
    tally = f32_bars.Tally("second", f"{name}/{which}")
    tally.add(which, reference, f32_bars.measure_second(reference, out))
    failures = tally.emit()
    assert not failures, failures


@pytest.mark.parametrize("name", list(f32_bars.TAYLOR))
def test_second_order_on_the_taylor_branches(device, name):
    """The oracle's H v is undefined on view 1's three zero-rotation entries (asserted to be the only such entries
    in tests/test_f32_bars.py); the kernel must be finite there, and nothing else is left out."""
    reference = f32_bars.second_reference(name, "both")
    expected = torch.zeros_like(reference.undefined)
    expected[:, f32_bars.rotation_entries(name, 1)] = True
    assert torch.equal(reference.undefined, expected)
    out = _second(device, name, "both")
    assert all(torch.isfinite(t).all() for t in out)
    tally = f32_bars.Tally("second_taylor", name)
    tally.add("both", reference, f32_bars.measure_second(reference, out))
    failures = tally.emit()
    assert not failures, failures
