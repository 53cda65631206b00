"""The HIP kernels against what the REFERENCE computed.

tests/golden/ref_stages_64x48.npz and ref_sequence_64x48.npz hold the outputs of the host build of the reference's own filter source
(oracle/ref_harness.cpp; recorded by tests/golden/make_golden.py where the reference checkout exists) next to the parameters that regenerate the
inputs (tests/reference_cases.py).  Every other GPU test ends at the CPU oracle, which this project wrote; these end at the reference's text.
Only tests/golden/ and the seeded generators are read — never the reference checkout or oracle/_ref.

64x48, fp16 storage (the reference's only one).  svgf_temporal: bit for bit.  svgf_moments, svgf_atrous, svgf_taa: the fp16 stage tolerance of
tests/gpu_helpers.py (TOL: at most one half-ulp, on at most 0.2 % of the values), identical NaN masks and infinities, sky texels copied bit for
bit, under the variants auto, direct and lds-general.  The frame driver's six frames: the free-running fp16 bounds of tests/helpers.py
(FREE_RUNNING, moving camera), history bit for bit."""
import os

import numpy as np
import pytest

from tests import reference_cases as rc
from tests.conftest import ROOT
from tests.helpers import free_running_bounds

pytestmark = pytest.mark.gpu

GOLD = os.path.join(ROOT, "tests", "golden")
VARIANTS = ["auto", "direct", "lds-general"]


@pytest.fixture(scope="module")
def G():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tests import gpu_helpers
    return gpu_helpers


def _load(name):
    z = np.load(os.path.join(GOLD, name))
    return {k[len("param_"):]: z[k] for k in z.files if k.startswith("param_")}, {k: z[k] for k in z.files if not k.startswith("param_")}


@pytest.fixture(scope="module")
def case():
    """The recorded reference outputs, and the inputs regenerated once from the recorded parameters."""
    params, want = _load("ref_stages_64x48.npz")
    return params, want, rc.fixture_inputs(params)


def _params(F, params, **kw):
    return F.Params(storage="f16", depth_threshold=float(params["depth_threshold"]), normal_threshold=float(params["normal_threshold"]),
                    history_base=int(params["history_base"]), mesh_id_test=int(params["mesh_id_test"]), phi_colour=float(params["phi_colour"]),
                    phi_normal=float(params["phi_normal"]), **kw)


def _held(G, got, want, what):
    """TOL["f16"] with identical NaN masks and infinities; the figures first"""
    from tests.helpers import half_ulp_diff
    from tests.test_gpu_nonfinite import assert_close_with_nan
    fin = np.isfinite(want.astype(np.float32)) & np.isfinite(got.astype(np.float32))
    d = half_ulp_diff(got[fin], want[fin])
    print(f"{what}: max {int(d.max())} half-ulps, {float((d > 0).mean()):.2e} of {d.size} values off, {int(np.isnan(want.astype(np.float32)).sum())} NaN")
    assert_close_with_nan(G, got, want, "f16", what)


def _sky(frame):
    z = frame["motion"][..., 2]
    return (z == 0) | (z == np.float32(1e30))


def test_temporal_is_the_reference_bit_for_bit(G, case):
    from svgf_amd import filter as F
    params, want, i = case
    W, H = i["W"], i["H"]
    prev, rad, hist, mom = i["temporal"]
    d = F.Denoiser(W, H, _params(F, params))
    o_col, o_hist, o_mom = d.new_colour(), d.new_history(), d.new_moments()
    d.TemporalFilter(G.dev(prev), G.dev(rad), o_col, G.gb_dev(i["f1"]), G.gb_dev(i["f0"]), G.dev(hist), o_hist, o_mom, G.dev(mom))
    assert np.array_equal(G.host(o_hist), want["temporal_hist"]), "history / accept-reject mask"
    assert 0.3 < (want["temporal_hist"] > 1).mean() < 1.0
    assert np.array_equal(G.host(o_col).view(np.uint16), want["temporal_colour"].view(np.uint16))
    assert np.array_equal(G.host(o_mom).view(np.uint16), want["temporal_mom"].view(np.uint16))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("tag", ["", "_poison"], ids=["clean", "poisoned"])
def test_moments(G, case, tag, variant):
    from svgf_amd import filter as F
    params, want, i = case
    W, H = i["W"], i["H"]
    (src, mom, hist, _), f = (i["spatial"], i["f1"]) if not tag else (i["spatial_poison"], i["p1"])
    d = F.Denoiser(W, H, _params(F, params, variant=variant))
    out = d.new_colour()
    d.FilterMoments(G.dev(src), out, G.dev(mom), G.gb_dev(f), G.dev(hist))
    got = G.host(out)
    keep = hist >= 4
    assert keep.any() and not keep.all()
    assert rc.same_bits(got[keep], want["moments" + tag][keep]).all(), "pass-through texels (history >= 4)"
    _held(G, got, want["moments" + tag], f"moments{tag} {variant}")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("which", [(1, 0, ""), (4, 1, ""), (1, 0, "_poison")], ids=["step1-it0", "step4-it1", "step1-it0-poisoned"])
def test_atrous(G, case, which, variant):
    from svgf_amd import filter as F
    params, want, i = case
    W, H = i["W"], i["H"]
    step, iteration, tag = which
    (src, _, _, marker), f = (i["spatial"], i["f1"]) if not tag else (i["spatial_poison"], i["p1"])
    name = f"atrous_step{step}_it{iteration}{tag}"
    d = F.Denoiser(W, H, _params(F, params, variant=variant))
    out, fb = d.new_colour(), G.dev(marker)
    d.FilterKernel(G.dev(src), out, fb if iteration == 0 else None, G.gb_dev(f), step, iteration)
    got, sky = G.host(out), _sky(f)
    assert sky.any() and not sky.all()
    assert rc.same_bits(got[sky], want[name][sky]).all(), "sky texels are copied"
    _held(G, got, want[name], f"{name} {variant}")
    if iteration == 0:
        got_fb = G.host(fb)
        assert np.array_equal(got_fb[sky].view(np.uint16), marker[sky].view(np.uint16)) and np.array_equal(want[name + "_feedback"][sky].view(np.uint16), marker[sky].view(np.uint16))
        _held(G, got_fb, want[name + "_feedback"], f"{name} feedback {variant}")


@pytest.mark.parametrize("variant", VARIANTS)
def test_taa(G, case, variant):
    from svgf_amd import filter as F
    params, want, i = case
    W, H = i["W"], i["H"]
    filt, hist = i["taa"]
    d = F.Denoiser(W, H, _params(F, params, variant=variant))
    out = d.new_colour()
    d.TAA(G.dev(filt), G.dev(hist), out)
    _held(G, G.host(out), want["taa"], f"taa {variant}")


def test_frame_driver_six_frames(G):
    """svgf_denoise_frame free running over the recorded sequence: the reference's final plane within the free-running fp16 bounds, its history exactly."""
    from svgf_amd import filter as F
    from svgf_amd import synth
    params, want = _load("ref_sequence_64x48.npz")
    W, H, N, steps = int(params["W"]), int(params["H"]), int(params["sequence_frames"]), int(params["sequence_steps"])
    mv = tuple(float(v) for v in params["mv"])
    fr = [synth.make_frame(W, H, k, mv=mv) for k in range(N)]
    gbs = [G.gb_dev(f) for f in fr]
    d = F.Denoiser(W, H, _params(F, params, steps=steps))
    for k in range(N):
        got = G.host(d.Render(G.dev(fr[k]["radiance"].astype(np.float16)), gbs[k], gbs[k - 1] if k else None))
    assert np.array_equal(G.host(d.state_plane(F.PLANE_HISTORY, 1 - d.pingpong())), want["hist"]), "history"
    b = free_running_bounds("f16", mv)
    w = want["out"].astype(np.float64)
    err = np.abs(got.astype(np.float64) - w)[..., :3]
    beyond = float((err > b["tight"] + 1e-5 * np.abs(w[..., :3])).mean())
    print(f"six frames: max err {err.max():.3e}, beyond tight {beyond:.2e}")
    assert err.max() <= b["loose"], f"max colour error {err.max():.3e}"
    assert beyond <= b["frac"]
