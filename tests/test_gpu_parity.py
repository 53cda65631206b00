"""GPU parity: the HIP kernels, called through the C ABI (include/svgf.h), against the CPU oracle on
the same seeded synthetic inputs.  Tolerances are stated in tests/gpu_helpers.py:TOL."""
import numpy as np
import pytest

from svgf_amd import synth
from tests.helpers import CDT, frames, free_running_bounds, free_running_envelope, gbuf

pytestmark = pytest.mark.gpu

VARIANTS = ["direct", "lds"]


@pytest.fixture(scope="module")
def G():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tests import gpu_helpers
    return gpu_helpers


@pytest.mark.parametrize("storage", ["f32", "f16"])
@pytest.mark.parametrize("mv", [(0.0, 0.0), (1.0, 0.0), (-2.5, 1.5)])
@pytest.mark.parametrize("mesh", [0, 1])
def test_temporal_bit_exact(G, oracle, storage, mv, mesh):
    from svgf_amd import filter as F
    W, H = 331, 203                                  # not multiples of the 64x4 launch tile
    rng = np.random.default_rng(1)
    f0, f1 = synth.make_frame(W, H, 3, mv=mv), synth.make_frame(W, H, 4, mv=mv)
    dt = CDT[storage]
    prev = rng.uniform(-0.1, 1.2, (H, W, 4)).astype(dt)
    mom_prev = rng.uniform(0, 1, (H, W, 2)).astype(dt)
    hist_prev = rng.integers(0, 40, (H, W)).astype(np.uint8)
    cur = (f1["radiance"] * 1.3 - 0.1).astype(dt)
    # the sign of a zero: the reference's clamp, built from comparisons, keeps -0.0 (Filter.cuh:57-82), so -0.0 x (1 - a) + -0.0 x a stays -0.0
    # (:398) and is stored as such (:401); whole rows of it in both frames (any reprojection lands on one), single channels elsewhere
    cur[40:52] = -0.0; prev[34:58] = -0.0
    cur[60:70, :, 1] = -0.0; prev[56:74, :, 1] = -0.0; cur[80:84, ::3, 2] = -0.0; prev[76:88, :, 2] = -0.0
    mom_prev[34:58] = -0.0
    out = np.zeros_like(cur); hist = np.zeros((H, W), np.uint8); mom = np.zeros((H, W, 2), dt)
    oracle.temporal(W, H, storage, prev, cur, out, gbuf(f1), gbuf(f0), hist_prev, hist, mom, mom_prev,
                    depth_threshold=0.8, normal_threshold=0.9, history_base=24, mesh_id_test=mesh)
    assert (out.view(np.uint32 if storage == "f32" else np.uint16) == (0x80000000 if storage == "f32" else 0x8000)).sum() > 1000, "the case holds no -0.0 result"
    d = F.Denoiser(W, H, F.Params(storage=storage, mesh_id_test=mesh))
    o_col, o_hist, o_mom = d.new_colour(), d.new_history(), d.new_moments()
    d.TemporalFilter(G.dev(prev), G.dev(cur), o_col, G.gb_dev(f1), G.gb_dev(f0), G.dev(hist_prev), o_hist, o_mom, G.dev(mom_prev))
    assert np.array_equal(G.host(o_hist), hist), "history / accept-reject mask mismatch"
    assert np.array_equal(G.host(o_col).view(np.uint8), out.view(np.uint8))
    assert np.array_equal(G.host(o_mom).view(np.uint8), mom.view(np.uint8))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("storage", ["f32", "f16"])
@pytest.mark.parametrize("radius", [3, 1])
def test_moments(G, oracle, storage, radius, variant):
    from svgf_amd import filter as F
    W, H = 203, 131
    rng = np.random.default_rng(2)
    f = synth.make_frame(W, H, 0)
    dt = CDT[storage]
    col = rng.uniform(0, 1, (H, W, 4)).astype(dt)
    mom = rng.uniform(0, 1, (H, W, 2)).astype(dt)
    hist = rng.integers(1, 8, (H, W)).astype(np.uint8)
    want = np.zeros_like(col)
    oracle.moments(W, H, storage, col, want, mom, gbuf(f), hist, phi_colour=10.0, phi_normal=128.0, radius=radius)
    d = F.Denoiser(W, H, F.Params(storage=storage, moments_radius=radius, variant=variant))   # lds: the streaming kernel (radius 3)
    out = d.new_colour()
    d.FilterMoments(G.dev(col), out, G.dev(mom), G.gb_dev(f), G.dev(hist))
    got = G.host(out)
    keep = hist >= 4
    assert np.array_equal(got[keep].view(np.uint8), col[keep].view(np.uint8))
    if storage == "f32":
        # variance here is a small difference of two weighted sums of O(1) moments: absolute tolerance
        g, w = got.astype(np.float64), want.astype(np.float64)
        assert np.abs(g[..., :3] - w[..., :3]).max() <= 2e-5
        assert np.abs(g[..., 3] - w[..., 3]).max() <= 2e-5 * 4
    else:
        G.assert_colour_close(got[..., :3], want[..., :3], storage, "moments colour")
        g, w = got[..., 3].astype(np.float64), want[..., 3].astype(np.float64)
        assert np.all(np.abs(g - w) <= 8e-5 + np.abs(w) * 2.0 ** -10)      # cancellation error + one half-ulp


@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_moments_3x3_wave_shuffle_kernel_is_bit_identical(G, storage):
    """moments_radius = 1: the wave64-shuffle kernel (default) against the per-pixel kernel (variant direct), bitwise, on
    widths around the 64-lane wave (edge lanes fetch the column beyond the wave) and through the frame driver's cold frames."""
    from svgf_amd import filter as F
    rng = np.random.default_rng(5)
    dt = CDT[storage]
    for (W, H) in ((203, 67), (64, 9), (65, 5), (1, 3), (129, 2)):
        f = synth.make_frame(W, H, 1)
        col = rng.uniform(0, 1, (H, W, 4)).astype(dt)
        mom = rng.uniform(0, 1, (H, W, 2)).astype(dt)
        hist = rng.integers(1, 7, (H, W)).astype(np.uint8)
        outs = []
        for variant in ("auto", "direct"):
            d = F.Denoiser(W, H, F.Params(storage=storage, moments_radius=1, variant=variant))
            o = d.new_colour()
            d.FilterMoments(G.dev(col), o, G.dev(mom), G.gb_dev(f), G.dev(hist))
            outs.append(G.host(o))
        assert np.array_equal(outs[0].view(np.uint8), outs[1].view(np.uint8)), (W, H)
    W, H = 200, 90
    fr = frames(W, H, 5, mv=(1.0, 0.0))
    gbs = [G.gb_dev(f) for f in fr]
    da = F.Denoiser(W, H, F.Params(storage=storage, steps=0, moments_radius=1))          # no iterations: the result IS the moments output
    dd = F.Denoiser(W, H, F.Params(storage=storage, steps=0, moments_radius=1, variant="direct"))
    for k in range(5):
        rad = G.dev(fr[k]["radiance"].astype(G.NPDT[storage]))
        a_ = G.host(da.Render(rad, gbs[k], gbs[k - 1] if k else None))
        b_ = G.host(dd.Render(rad, gbs[k], gbs[k - 1] if k else None))
        assert np.array_equal(a_.view(np.uint8), b_.view(np.uint8)), f"driver radius 1 frame {k}"
        assert np.array_equal(G.host(da.state_plane(F.PLANE_HISTORY, 1 - da.pingpong())), G.host(dd.state_plane(F.PLANE_HISTORY, 1 - dd.pingpong())))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("storage", ["f32", "f16"])
@pytest.mark.parametrize("step", [1, 2, 4, 8, 16])
def test_atrous(G, oracle, storage, step, variant):
    from svgf_amd import filter as F
    W, H = 333, 207
    rng = np.random.default_rng(3 + step)
    f = synth.make_frame(W, H, 0)
    dt = CDT[storage]
    src = np.concatenate([f["radiance"][..., :3] * 1.2 - 0.05, rng.uniform(-0.01, 0.05, (H, W, 1)).astype(np.float32)], -1).astype(dt)
    # -0.0 channels: a sky texel is copied with the sign of its zeros (the reference's clamp keeps it, Filter.cuh:57-82,554-558); a surface
    # texel's sums lose it unless every tap holds it too (a whole block does)
    sky = f["region"] == synth.SKY
    ys, xs = np.nonzero(sky)
    assert len(ys) > 200
    src[ys[::5], xs[::5]] = -0.0
    src[ys[1::5], xs[1::5], rng.integers(0, 4, len(ys[1::5]))] = -0.0
    sy, sx = np.nonzero(~sky)
    src[sy[::41], sx[::41], rng.integers(0, 4, len(sy[::41]))] = -0.0
    src[100:140, 150:200, 1] = -0.0
    want = np.zeros_like(src); want_fb = np.full_like(src, 7)
    oracle.atrous(W, H, storage, src, want, want_fb, gbuf(f), step=step, phi_colour=10.0, phi_normal=128.0, iteration=0)
    u = np.uint32 if storage == "f32" else np.uint16
    assert (want[sky].view(u) == (0x80000000 if storage == "f32" else 0x8000)).sum() > 100, "the case holds no -0.0 sky texel"
    d = F.Denoiser(W, H, F.Params(storage=storage, variant=variant))
    out = d.new_colour(); fb = G.dev(np.full_like(src, 7))
    d.FilterKernel(G.dev(src), out, fb, G.gb_dev(f), step, 0)
    got, got_fb = G.host(out), G.host(fb)
    G.assert_colour_close(got, want, storage, f"atrous step {step} {variant}")
    assert np.array_equal(got[sky].view(np.uint8), want[sky].view(np.uint8))            # clamped copy, exact: raw bits, the sign of a zero included
    zero = want == 0                                                                     # ... and a filtered zero carries the reference's sign too
    if step == 1:
        assert (np.signbit(want[zero]) & ~sky[..., None].repeat(4, -1)[zero]).sum() > 1000, "the case holds no filtered -0.0"
    assert np.array_equal(got[zero] == 0, want[zero] == 0) and np.array_equal(np.signbit(got[zero]), np.signbit(want[zero]))
    assert np.all(got_fb[sky] == 7)                                                      # no feedback on sky
    assert np.array_equal(got_fb[~sky].view(np.uint8), got[~sky].view(np.uint8))
    out2 = d.new_colour(); fb2 = G.dev(np.full_like(src, 7))
    d.FilterKernel(G.dev(src), out2, fb2, G.gb_dev(f), step, 1)                          # iteration != 0: no feedback
    assert np.all(G.host(fb2) == 7)
    assert np.array_equal(G.host(out2).view(np.uint8), got.view(np.uint8))


@pytest.mark.parametrize("seed", range(8))
def test_random_tunables_and_sizes_vs_oracle(G, oracle, seed):
    """Seeded sweep over the GUI ranges of the tunables (GUI.cpp:988-993) and over frame sizes: a-trous (LDS kernel) and
    temporal from identical random inputs against the oracle."""
    from svgf_amd import filter as F
    rng = np.random.default_rng(100 + seed)
    W, H = int(rng.integers(65, 420)), int(rng.integers(9, 200))
    storage = ("f32", "f16")[seed & 1]
    dt = CDT[storage]
    step = int(2 ** rng.integers(0, 5))
    phi_c, phi_n = float(rng.uniform(0.05, 40.0)), float(rng.uniform(0.5, 256.0))
    dthr, nthr, hb = float(rng.uniform(0.0, 3.0)), float(rng.uniform(0.0, 1.0)), int(rng.integers(1, 256))
    mv = (float(rng.uniform(-3, 3)), float(rng.uniform(-3, 3)))
    f0, f1 = synth.make_frame(W, H, seed, mv=mv), synth.make_frame(W, H, seed + 1, mv=mv)
    # a-trous
    src = np.concatenate([rng.uniform(-0.2, 1.3, (H, W, 3)), rng.uniform(-0.01, 0.2, (H, W, 1))], -1).astype(dt)
    want = np.zeros_like(src); fbw = np.zeros_like(src)
    oracle.atrous(W, H, storage, src, want, fbw, gbuf(f1), step=step, phi_colour=phi_c, phi_normal=phi_n, iteration=0)
    d = F.Denoiser(W, H, F.Params(storage=storage, phi_colour=phi_c, phi_normal=phi_n, depth_threshold=dthr, normal_threshold=nthr,
                                  history_base=hb, variant="lds"))
    out, fb = d.new_colour(), d.new_colour()
    d.FilterKernel(G.dev(src), out, fb, G.gb_dev(f1), step, 0)
    G.assert_colour_close(G.host(out), want, storage, f"seed {seed}: {W}x{H} step {step} phi {phi_c:.2f}/{phi_n:.1f}")
    # temporal: bit-exact whatever the thresholds
    prev = rng.uniform(-0.1, 1.2, (H, W, 4)).astype(dt)
    mom_prev = rng.uniform(0, 1, (H, W, 2)).astype(dt)
    hist_prev = rng.integers(0, 256, (H, W)).astype(np.uint8)
    cur = rng.uniform(-0.1, 1.4, (H, W, 4)).astype(dt)
    o = np.zeros_like(cur); hist = np.zeros((H, W), np.uint8); mom = np.zeros((H, W, 2), dt)
    oracle.temporal(W, H, storage, prev, cur, o, gbuf(f1), gbuf(f0), hist_prev, hist, mom, mom_prev,
                    depth_threshold=dthr, normal_threshold=nthr, history_base=hb, mesh_id_test=1)
    o_col, o_hist, o_mom = d.new_colour(), d.new_history(), d.new_moments()
    d.TemporalFilter(G.dev(prev), G.dev(cur), o_col, G.gb_dev(f1), G.gb_dev(f0), G.dev(hist_prev), o_hist, o_mom, G.dev(mom_prev))
    assert np.array_equal(G.host(o_hist), hist)
    assert np.array_equal(G.host(o_col).view(np.uint8), o.view(np.uint8))
    assert np.array_equal(G.host(o_mom).view(np.uint8), mom.view(np.uint8))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("storage", ["f32", "f16"])
@pytest.mark.parametrize("mv", [(0.0, 0.0), (-2.5, 1.5)])
def test_pipeline_stagewise_identical_inputs(G, oracle, storage, mv, variant):
    """8 frames with history feedback; every device stage of every frame is fed the ORACLE's inputs for that
    stage (bit-identical inputs) and must match the oracle's output within the stage tolerance.  This is the
    parity statement proper: SURVEY.md App. A.6."""
    from svgf_amd import filter as F
    W, H, N = 256, 144, 8
    fr = frames(W, H, N, mv=mv)
    ref = oracle.Pipeline(W, H, storage, steps=5, nthreads=8)
    d = F.Denoiser(W, H, F.Params(storage=storage, steps=5, variant=variant))
    gbs = [G.gb_dev(f) for f in fr]
    for k in range(N):
        kp = max(k - 1, 0)
        ref.frame(fr[k]["radiance"], gbuf(fr[k]), gbuf(fr[kp]))
        t = ref.taps
        col, hist, mom = d.new_colour(), d.new_history(), d.new_moments()
        d.TemporalFilter(G.dev(t["prev_colour"]), G.dev(t["radiance"]), col, gbs[k], gbs[kp], G.dev(t["prev_hist"]), hist,
                         mom, G.dev(t["prev_mom"]))
        assert np.array_equal(G.host(hist), t["hist"]), f"frame {k}: history mask mismatch"
        assert np.array_equal(G.host(col).view(np.uint8), t["temporal"].view(np.uint8)), f"frame {k}: temporal colour"
        assert np.array_equal(G.host(mom).view(np.uint8), t["mom"].view(np.uint8)), f"frame {k}: temporal moments"
        out = d.new_colour()
        d.FilterMoments(G.dev(t["temporal"]), out, G.dev(t["mom"]), gbs[k], G.dev(t["hist"]))
        got, want = G.host(out), t["moments"]
        if storage == "f32":
            assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 8e-5, f"frame {k}: moments"
        else:
            assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 1e-3, f"frame {k}: moments"
        for i in range(5):
            fb = G.dev(t["temporal"]) if i == 0 else None
            d.FilterKernel(G.dev(t["atrous_in"][i]), out, fb, gbs[k], 1 << i, i)
            G.assert_colour_close(G.host(out), t["atrous_out"][i], storage, f"frame {k} a-trous iteration {i}")
            if i == 0:
                assert np.array_equal(G.host(fb).view(np.uint8)[fr[k]["region"] == synth.SKY],
                                      t["temporal"].view(np.uint8)[fr[k]["region"] == synth.SKY])


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("storage", ["f32", "f16"])
@pytest.mark.parametrize("mv", [(0.0, 0.0), (-2.5, 1.5)])
def test_pipeline_free_running(G, oracle, storage, mv, variant):
    """The same 8 frames free-running (device feeds itself).  Accept/reject masks must stay identical.  Colour is
    compared in two tiers because the reference algorithm is ill-conditioned where the temporal variance is
    exactly 0 (phi_l = PhiColour*sqrt(1e-10) = 1e-4, Filter.cuh:562): there a 1-ulp difference in an INPUT
    luminance moves a weight by ~1e-3, so two correct fp32 implementations (e.g. nvcc with and without FMA
    contraction) differ by ~1e-4 on a few pixels once their inputs differ by an ulp ('Tolerance')."""
    W, H, N = 256, 144, 8
    fr = frames(W, H, N, mv=mv)
    ref = oracle.Pipeline(W, H, storage, steps=5, nthreads=8)
    hip = G.HipPipeline(W, H, storage, steps=5, variant=variant)
    gbs = [G.gb_dev(f) for f in fr]
    # measured on MI355X (profiles/r0N_parity_report.json, tools/archive/diag_free.py): f32 max 2.5e-4 with < 1e-3 of the values beyond 2e-5;
    # f16 max 1.0e-2 (static camera, frame 3: ten half-ulps at 0.5-1.0 on a handful of pixels) with < 1e-4 of the values beyond 1e-3 —
    # all in frames 3-4, where the first pixels leave the spatial variance estimate.  The bounds are 2x the measured maxima
    # (tests/helpers.py:FREE_RUNNING) — and, round 5, the measured ENVELOPE of the same frames: the distance between two correct CPU
    # implementations of the reference's source (the oracle and its all-fp32 + FMA build).
    b = free_running_bounds(storage, mv)
    tight, loose, frac = b["tight"], b["loose"], b["frac"]
    worst = 0.0
    for k in range(N):
        kp = max(k - 1, 0)
        want = ref.frame(fr[k]["radiance"], gbuf(fr[k]), gbuf(fr[kp])).astype(np.float64)
        got = hip.frame(fr[k]["radiance"], gbs[k], gbs[kp]).astype(np.float64)
        assert np.array_equal(hip.taps["hist"], ref.taps["hist"]), f"frame {k}: history mask mismatch"
        err = np.abs(got - want)[..., :3]
        worst = max(worst, float(err.max()))
        assert err.max() <= loose, f"frame {k}: max colour error {err.max():.3e}"
        assert (err > tight + 1e-5 * np.abs(want[..., :3])).mean() <= frac, f"frame {k}: {(err > tight).mean():.2e} of values beyond the tight tolerance"
    env = free_running_envelope(oracle, fr, storage, flavour=b["inside_envelope"])      # (fp16 under a pan: the 1-ulp transcendental model, tests/helpers.py)
    assert env["mask_mismatches"] == 0
    assert worst <= env["max_abs"], f"HIP-vs-oracle {worst:.3e} is outside oracle-vs-oracle' ({b['inside_envelope']}) {env['max_abs']:.3e}"


@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_frame_driver_equals_stage_calls(G, storage):
    """svgf_denoise_frame (context-owned state, moments pass-through folded into the temporal launch) == the same
    stages driven from outside, bitwise — here with variant "direct" (the per-pixel kernels; the default variants, whose young-pixel
    launch and LDS-streaming moments kernel evaluate the estimate on the same bits, are compared the same way in test_gpu_fused.py)."""
    from svgf_amd import filter as F
    W, H, N = 200, 120, 6
    fr = frames(W, H, N, mv=(1.0, 0.0))
    hip = G.HipPipeline(W, H, storage, steps=3, variant="direct")
    d = F.Denoiser(W, H, F.Params(storage=storage, steps=3, variant="direct"))
    gbs = [G.gb_dev(f) for f in fr]
    for k in range(N):
        kp = max(k - 1, 0)
        a = hip.frame(fr[k]["radiance"], gbs[k], gbs[kp])
        b = G.host(d.Render(G.dev(fr[k]["radiance"].astype(G.NPDT[storage])), gbs[k], gbs[kp] if k else None))
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), k
    assert d.pingpong() == N % 2
    assert np.array_equal(G.host(d.state_plane(F.PLANE_HISTORY, 1 - d.pingpong())), hip.taps["hist"])


@pytest.mark.parametrize("period,storage", [(8, "f32"), (2, "f16"), (64, "f32")])
def test_frame_driver_when_every_wave_holds_young_pixels(G, period, storage):
    """Thin geometry under motion: every `period`-th column fails the reprojection test in every frame (the two G-buffers the frames
    alternate between disagree on its normals), so EVERY wave of the temporal launch holds young pixels — more waves than the young
    list takes appends from (svgf_kernels.h: young_append_cap = a quarter of the waves, an eighth of that per shard).  The temporal launch stops appending and the moments launch
    works from the per-segment masks: still the stage sequence's results, bit for bit."""
    from svgf_amd import filter as F
    W, H, N = 2048, 800, 6                                  # 32 x 800 = 25 600 waves, ~8 % of them sky
    fr = frames(W, H, 2, mv=(0.0, 0.0))
    gbn = []
    for k in (0, 1):
        n = fr[0]["normal"].copy()
        if k:
            n.view(np.int16)[:, ::period, 0:3] ^= np.int16(-32768)      # the sign of the normal, in one of the two G-buffers
        gbn.append(G.F.GBuffer(G.dev(fr[0]["motion"]), G.dev(n), G.dev(fr[0]["uv"])))
    hip = G.HipPipeline(W, H, storage, steps=3, variant="direct")
    d = F.Denoiser(W, H, F.Params(storage=storage, steps=3, variant="direct"))
    for k in range(N):
        rad = fr[k % 2]["radiance"]
        a = hip.frame(rad, gbn[k % 2], gbn[(k + 1) % 2] if k else gbn[0])
        b = G.host(d.Render(G.dev(rad.astype(G.NPDT[storage])), gbn[k % 2], gbn[(k + 1) % 2] if k else None))
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), k
    hist = G.host(d.state_plane(F.PLANE_HISTORY, 1 - d.pingpong()))
    assert np.array_equal(hist, hip.taps["hist"])
    surface = fr[0]["motion"][..., 2] != 0
    assert (hist[:, ::period][surface[:, ::period]] == 1).all() and (hist[:, 1::period][surface[:, 1::period]] >= 4).mean() > 0.9


@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_adaptive_moments_switches_kernels_without_a_bit_changing(G, storage):
    """A sequence that goes from calm to crowded and back (every 8th column disoccluded in every frame of the middle part: 12 % of the
    surface pixels young): with the host waiting for every frame the sample of frame f reaches the driver at frame f + 2, which then
    serves the young pixels with the LDS-streaming kernel instead of the young-pixel launch, and goes back when the frames calm down.
    The frames equal those of a context that never switches, bit for bit."""
    import torch
    from svgf_amd import filter as F
    W, H, N = 1024, 512, 22
    fr = frames(W, H, 2, mv=(0.0, 0.0))
    base = fr[0]["normal"]
    flipped = base.copy()
    flipped.view(np.int16)[:, ::8, 0:3] ^= np.int16(-32768)
    mot, uv = G.dev(fr[0]["motion"]), G.dev(fr[0]["uv"])
    calm = [G.F.GBuffer(mot, G.dev(base), uv), G.F.GBuffer(mot, G.dev(base.copy()), uv)]
    crowd = [calm[0], G.F.GBuffer(mot, G.dev(flipped), uv)]
    gb_of = lambda k: (crowd if 8 <= k < 15 else calm)[k % 2]          # noqa: E731
    outs, modes = {}, []
    for adaptive in (True, False):
        d = F.Denoiser(W, H, F.Params(storage=storage, steps=3))
        d.set_adaptive_moments(adaptive)
        res = []
        for k in range(N):
            rad = G.dev(fr[k % 2]["radiance"].astype(G.NPDT[storage]))
            res.append(G.host(d.Render(rad, gb_of(k), gb_of(k - 1) if k else None)))      # (G.host waits for the frame)
            if adaptive:
                modes.append(d.adaptive_moments_state())
                if k == 14:         # the sample the driver reads: one wave in 64 of a frame two calls ago, x 64 (svgf_adaptive_moments_sample)
                    px, waves = d.adaptive_moments_sample()
                    hist = G.host(d.state_plane(F.PLANE_HISTORY, 1 - d.pingpong()))
                    surface = fr[0]["motion"][..., 2] != 0
                    young = int(((hist < 4) & surface).sum())
                    assert 0.6 * young < px < 1.4 * young and waves > 0.5 * (H * W // 64), (px, waves, young)
        outs[adaptive] = res
        d.close()
    # frames 0-2 are young all over (the streaming kernel serves them whatever the sample says, and they add nothing to it), 9-15 crowded
    # (frame 9 is the first whose two G-buffers disagree; seen from frame 11 on), 18 is the first calm one again (seen at frame 20)
    assert not any(modes[:9]) and all(modes[11:17]) and not modes[-1], modes
    for k in range(N):
        assert np.array_equal(outs[True][k].view(np.uint8), outs[False][k].view(np.uint8)), k


@pytest.mark.parametrize("params", [
    dict(steps=0), dict(steps=1), dict(steps=5, phi_normal=0.0), dict(steps=3, history_base=2), dict(steps=3, history_base=4),
    dict(steps=2, mesh_id_test=0, normal_threshold=0.0), dict(steps=3, moments_radius=1), dict(steps=4, depth_threshold=0.0, phi_colour=0.5),
])
def test_frame_driver_fusions_hold_for_any_parameters(G, params):
    """The driver's fusions (moments copy and exact sky zeros written by the temporal launch, young-segment flags, the
    temporal result stored only where iteration 0's feedback will not overwrite it) are bit-identical to the plain stage
    sequence whatever the tunables: no iteration at all, PhiNormal = 0 (no sky shortcut), a history cap below / at the
    'young' limit of 4, thresholds that accept everything, the 3x3 estimate."""
    from svgf_amd import filter as F
    W, H, N = 203, 77, 7
    fr = frames(W, H, N, mv=(-2.5, 1.5))
    for storage in ("f32", "f16"):
        hip = G.HipPipeline(W, H, storage, variant="direct", **params)
        d = F.Denoiser(W, H, F.Params(storage=storage, variant="direct", **params))
        gbs = [G.gb_dev(f) for f in fr]
        for k in range(N):
            kp = max(k - 1, 0)
            a = hip.frame(fr[k]["radiance"], gbs[k], gbs[kp])
            b = G.host(d.Render(G.dev(fr[k]["radiance"].astype(G.NPDT[storage])), gbs[k], gbs[kp] if k else None))
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (storage, k)
        assert np.array_equal(G.host(d.state_plane(F.PLANE_HISTORY, 1 - d.pingpong())), hip.taps["hist"])
        assert np.array_equal(G.host(d.state_plane(F.PLANE_MOMENTS, 1 - d.pingpong())).view(np.uint8), hip.taps["mom"].view(np.uint8))


@pytest.mark.parametrize("params", [
    dict(steps=3, moments_radius=0), dict(steps=3, moments_radius=2), dict(steps=3, phi_normal=0.0), dict(steps=2, moments_radius=1),
    dict(steps=3, moments_radius=2, variant="lds"),
])
def test_frame_driver_first_frames_under_the_default_variants(G, params):
    """in the first three frames after a reset the frame driver called every frame "cold" under variant auto / lds —
    its temporal launch then appends to no young list — while launch_moments only has an every-pixel kernel for the reference's radius
    with PhiNormal != 0 (LDS streaming) and for radius 1 (wave shuffles).  With radius 0 / 2 or PhiNormal == 0 the young-pixel launch
    ran without its list: the young pixels of partly young 64-column segments (sky silhouettes; the right-most segment when W % 64 != 0)
    kept stale filter_out texels.  W = 203 (W % 64 = 11), a scene with sky, a reset in mid-sequence; bitwise against the stage calls."""
    from svgf_amd import filter as F
    W, H, N = 203, 77, 9
    fr = frames(W, H, N, mv=(-2.5, 1.5))
    p = dict(variant="auto")
    p.update(params)
    for storage in ("f32", "f16"):
        hip = G.HipPipeline(W, H, storage, **p)
        d = F.Denoiser(W, H, F.Params(storage=storage, **p))
        gbs = [G.gb_dev(f) for f in fr]
        for k in range(N):
            if k == 5:                                   # a reset in mid-sequence: three more cold frames, on planes that hold stale data
                d.reset_history()
                for t in hip.colour + hip.mom + hip.hist:
                    t.zero_()
                hip.filt[0].fill_(0.25)                  # (the stage calls overwrite every texel; the driver's planes are zeroed by the reset)
            kp = max(k - 1, 0)
            a = hip.frame(fr[k]["radiance"], gbs[k], gbs[kp])
            b = G.host(d.Render(G.dev(fr[k]["radiance"].astype(G.NPDT[storage])), gbs[k], gbs[kp] if k else None))
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (storage, k)
        assert np.array_equal(G.host(d.state_plane(F.PLANE_HISTORY, 1 - d.pingpong())), hip.taps["hist"])


@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_temporal_moments_fused_equals_stage_calls(G, storage):
    """svgf_temporal_moments (caller-owned planes; the strip runner's path) == svgf_temporal + svgf_moments, bitwise,
    over the cold -> steady transition, with the moments rows a sub-range of the temporal rows."""
    from svgf_amd import filter as F
    W, H, N = 200, 120, 7
    fr = frames(W, H, N, mv=(-2.5, 1.5))
    hip = G.HipPipeline(W, H, storage, steps=0)
    d = F.Denoiser(W, H, F.Params(storage=storage, steps=0))
    colour, mom, hist = [d.new_colour() for _ in range(2)], [d.new_moments() for _ in range(2)], [d.new_history() for _ in range(2)]
    filt = d.new_colour()
    gbs = [G.gb_dev(f) for f in fr]
    mrows = (8, H - 5)
    for k in range(N):
        P, kp = k & 1, max(k - 1, 0)
        hip.frame(fr[k]["radiance"], gbs[k], gbs[kp])
        rad = G.dev(fr[k]["radiance"].astype(G.NPDT[storage]))
        d.TemporalMoments(colour[1 - P], rad, colour[P], filt, gbs[k], gbs[kp], hist[1 - P], hist[P], mom[P], mom[1 - P], mrows)
        assert np.array_equal(G.host(colour[P]).view(np.uint8), hip.taps["temporal"].view(np.uint8)), k
        assert np.array_equal(G.host(mom[P]).view(np.uint8), hip.taps["mom"].view(np.uint8)), k
        assert np.array_equal(G.host(hist[P]), hip.taps["hist"]), k
        assert np.array_equal(G.host(filt)[mrows[0]:mrows[1]].view(np.uint8), hip.taps["moments"][mrows[0]:mrows[1]].view(np.uint8)), k
    with pytest.raises(F.SvgfError):
        d.TemporalMoments(colour[0], rad, colour[1], colour[1], gbs[0], gbs[0], hist[0], hist[1], mom[1], mom[0])      # filter_out aliases colour_out
    with pytest.raises(F.SvgfError):
        d.TemporalMoments(colour[0], rad, colour[1], filt, gbs[0], gbs[0], hist[0], hist[1], mom[1], mom[0], (-3, H))     # rows outside


@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_frame_driver_default_path(G, oracle, storage):
    """The default driver (LDS moments kernel while history < 4 everywhere, fused pass-through afterwards, LDS
    à-trous) against the oracle, free running over the cold -> steady transition."""
    from svgf_amd import filter as F
    W, H, N = 256, 144, 8
    fr = frames(W, H, N, mv=(-2.5, 1.5))
    ref = oracle.Pipeline(W, H, storage, steps=5, nthreads=8)
    d = F.Denoiser(W, H, F.Params(storage=storage, steps=5))
    gbs = [G.gb_dev(f) for f in fr]
    b = free_running_bounds(storage, (-2.5, 1.5))          # 2x the maxima measured on MI355X (see test_pipeline_free_running)
    tight, loose, frac = b["tight"], b["loose"], b["frac"]
    for k in range(N):
        kp = max(k - 1, 0)
        want = ref.frame(fr[k]["radiance"], gbuf(fr[k]), gbuf(fr[kp])).astype(np.float64)
        got = G.host(d.Render(G.dev(fr[k]["radiance"].astype(G.NPDT[storage])), gbs[k], gbs[kp] if k else None)).astype(np.float64)
        assert np.array_equal(G.host(d.state_plane(F.PLANE_HISTORY, 1 - d.pingpong())), ref.taps["hist"]), f"frame {k}: history"
        err = np.abs(got - want)[..., :3]
        assert err.max() <= loose, f"frame {k}: max colour error {err.max():.3e}"
        assert (err > tight + 1e-5 * np.abs(want[..., :3])).mean() <= frac, f"frame {k}"
    d.reset_history()
    want0 = oracle.Pipeline(W, H, storage, steps=5, nthreads=8).frame(fr[0]["radiance"], gbuf(fr[0]), gbuf(fr[0]))
    got0 = G.host(d.Render(G.dev(fr[0]["radiance"].astype(G.NPDT[storage])), gbs[0], None))
    assert np.abs(got0.astype(np.float64) - want0.astype(np.float64)).max() <= loose      # reset_history restarts the cold path


@pytest.mark.parametrize("variant", VARIANTS)
def test_strips_bitwise_equal_whole_frame(G, variant):
    """Row strips with halo (virtual ranks on one device) reproduce the whole-frame à-trous bit for bit."""
    from svgf_amd import filter as F
    W, H, step = 320, 240, 8
    f = synth.make_frame(W, H, 0)
    src = f["radiance"].copy(); src[..., 3] = 0.02
    whole = F.Denoiser(W, H, F.Params(storage="f32", variant=variant))
    out = whole.new_colour()
    whole.FilterKernel(G.dev(src), out, None, G.gb_dev(f), step, 1)
    want = G.host(out)
    for (yb, ye) in [(0, 60), (60, 180), (180, 240)]:
        halo = 2 * step
        y0, y1 = max(0, yb - halo), min(H, ye + halo)
        loc = {k: np.ascontiguousarray(v[y0:y1]) for k, v in f.items() if k != "region"}
        d = F.Denoiser(W, H, F.Params(storage="f32", variant=variant), strip=(y0, y1 - y0, yb, ye))
        o = d.new_colour()
        d.FilterKernel(G.dev(np.ascontiguousarray(src[y0:y1])), o, None, G.gb_dev(loc), step, 1)
        assert np.array_equal(G.host(o)[yb - y0:ye - y0], want[yb:ye]), (yb, ye)


def test_abi_errors(G):
    from svgf_amd import filter as F
    W, H = 64, 48
    f = synth.make_frame(W, H, 0)
    d = F.Denoiser(W, H, F.Params(storage="f32"), strip=(8, 24, 16, 24))
    gb = G.gb_dev({k: v[8:32] for k, v in f.items() if k != "region"})
    a, b = d.new_colour(), d.new_colour()
    with pytest.raises(F.SvgfError, match="halo"):
        d.FilterKernel(a, b, None, gb, 8, 1)                     # needs 16 halo rows, strip holds 8
    with pytest.raises(F.SvgfError, match="in-place"):
        d.FilterKernel(a, a, None, gb, 1, 1)
    with pytest.raises(F.SvgfError, match="null"):
        d.FilterKernel(None, b, None, gb, 1, 1)
    with pytest.raises(F.SvgfError, match="step"):
        d.FilterKernel(a, b, None, gb, 0, 1)
    d.FilterKernel(a, b, None, gb, 4, 1)                         # 8 halo rows: fine


# ------------------------------------------------------------------ full-size properties ------
@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_4k_properties(G, storage):
    """Size-independent properties at BASELINE's 3840x2160 (each stage against the oracle at this size, in its long-band launch geometry:
    tests/test_gpu_fullsize_parity.py): (1) all-sky frame -> clamped copy; (2) uniform colour on a flat surface is a fixed point of the colour
    channels and variance follows v(1+sum g^2)/(1+sum g)^2; (3) two strips tile the whole frame bitwise."""
    import torch
    from svgf_amd import filter as F
    W, H = 3840, 2160
    dt = torch.float32 if storage == "f32" else torch.float16
    d = F.Denoiser(W, H, F.Params(storage=storage))
    motion = torch.zeros((H, W, 4), device="cuda"); normal = torch.zeros((H, W, 4), dtype=torch.int16, device="cuda")
    uv = torch.zeros_like(normal)
    gb_sky = F.GBuffer(motion, normal, uv)
    g = torch.Generator(device="cuda").manual_seed(5)
    src = (torch.rand((H, W, 4), device="cuda", generator=g) * 2 - 0.5).to(dt)
    out = d.new_colour()
    d.FilterKernel(src, out, None, gb_sky, 4, 1)
    assert torch.equal(out, src.clamp(0, 1))

    motion2 = motion.clone(); motion2[..., 2] = 5.0; motion2[..., 3] = 0.01
    normal2 = normal.clone(); normal2[..., 2] = int(np.float16(-1.0).view(np.int16))
    gb_flat = F.GBuffer(motion2, normal2, uv)
    src2 = torch.empty((H, W, 4), device="cuda", dtype=dt); src2[...] = torch.tensor([0.25, 0.5, 0.75, 0.125], dtype=dt)
    for step in (1, 16):
        d.FilterKernel(src2, out, None, gb_flat, step, 1)
        m = 2 * step
        inner = out[m:-m, m:-m].float()
        K = np.array([1.0, 2 / 3, 1 / 6]); gk = np.outer(K[[2, 1, 0, 1, 2]], K[[2, 1, 0, 1, 2]]); gk[2, 2] = 0
        want_var = 0.125 * (1 + (gk ** 2).sum()) / (1 + gk.sum()) ** 2
        tol = 2e-6 if storage == "f32" else 1e-3
        assert (inner[..., :3] - torch.tensor([0.25, 0.5, 0.75], device="cuda")).abs().max().item() <= tol
        assert (inner[..., 3] - want_var).abs().max().item() <= (1e-6 if storage == "f32" else 1e-4)

    fr = synth.make_frame(W, H, 0)
    gbw = G.gb_dev(fr)
    srcw = G.dev(fr["radiance"].astype(G.NPDT[storage]))
    d.FilterKernel(srcw, out, None, gbw, 16, 1)
    for (yb, ye) in [(0, 1080), (1080, 2160)]:
        y0, y1 = max(0, yb - 32), min(H, ye + 32)
        ds = F.Denoiser(W, H, F.Params(storage=storage), strip=(y0, y1 - y0, yb, ye))
        gl = F.GBuffer(gbw.motion[y0:y1].contiguous(), gbw.normal[y0:y1].contiguous(), gbw.uv[y0:y1].contiguous())
        o = ds.new_colour()
        ds.FilterKernel(srcw[y0:y1].contiguous(), o, None, gl, 16, 1)
        assert torch.equal(o[yb - y0:ye - y0], out[yb:ye])


def test_1080p_history_counts(G):
    """Static camera at 1920x1080: history is min(k, HistoryLength) on surfaces, 1 on sky."""
    import torch
    from svgf_amd import filter as F
    W, H, base = 1920, 1080, 5
    fr = synth.make_frame(W, H, 0)
    d = F.Denoiser(W, H, F.Params(storage="f16", steps=5, history_base=base))
    gb = G.gb_dev(fr)
    rad = G.dev(fr["radiance"].astype(np.float16))
    sky = torch.from_numpy(fr["region"] == synth.SKY).cuda()
    for k in range(7):
        out = d.Render(rad, gb, gb)
        h = d.state_plane(F.PLANE_HISTORY, 1 - d.pingpong())
        assert torch.all(h[~sky] == min(k + 1, base)) and torch.all(h[sky] == 1)
        assert torch.isfinite(out.float()).all()


@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_taa(G, oracle, storage):
    """The stage after the path: TAA + sRGB, two chained frames, against the oracle."""
    from svgf_amd import filter as F
    W, H = 333, 207
    rng = np.random.default_rng(31)
    dt = CDT[storage]
    f = synth.make_frame(W, H, 0)
    frames_ = [np.concatenate([f["base"] * s, np.ones((H, W, 1), np.float32)], -1).astype(dt) for s in (1.0, 1.3)]
    hist = rng.uniform(0, 1, (H, W, 4)).astype(dt)
    d = F.Denoiser(W, H, F.Params(storage=storage))
    h_dev = G.dev(hist)
    for fr in frames_:
        want = np.zeros_like(fr)
        oracle.taa(W, H, storage, fr, hist, want)
        out = d.new_colour()
        d.TAA(G.dev(fr), h_dev, out)
        got = G.host(out)
        if storage == "f32":
            assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 2e-6      # hardware exp2/log2 in sRGB
        else:
            from tests.helpers import half_ulp_diff
            assert half_ulp_diff(got, want).max() <= 1
        hist, h_dev = want, G.dev(want)
    with pytest.raises(F.SvgfError, match="in-place"):
        d.TAA(h_dev, h_dev, h_dev)
    # the LDS-tiled kernel (default) and the per-pixel kernel (variant direct) are bit-identical, also at a size where the
    # fp32 rounding of uv*(N-1) moves some samples one more texel up-left
    for (w2, h2) in ((W, H), (3840, 70), (517, 2160 // 8)):
        a_, b_ = rng.uniform(-0.1, 1.2, (h2, w2, 4)).astype(dt), rng.uniform(0, 1, (h2, w2, 4)).astype(dt)
        d1, d2 = F.Denoiser(w2, h2, F.Params(storage=storage)), F.Denoiser(w2, h2, F.Params(storage=storage, variant="direct"))
        o1, o2 = d1.new_colour(), d2.new_colour()
        d1.TAA(G.dev(a_), G.dev(b_), o1)
        d2.TAA(G.dev(a_), G.dev(b_), o2)
        assert np.array_equal(G.host(o1).view(np.uint8), G.host(o2).view(np.uint8)), (w2, h2)


@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_atrous_large_steps_and_degenerate_phis(G, oracle, storage):
    """GUI ranges (src/GUI.cpp:988-993): up to 10 iterations (steps 32..512 take the direct kernel), PhiNormal = 0
    (pow(x,0) = 1 also at x = 0) and PhiColour = 0 (|dl|/0: inf, or NaN -> 0 through fmax, Filter.cuh:422-424)."""
    from svgf_amd import filter as F
    W, H = 300, 180
    rng = np.random.default_rng(77)
    f = synth.make_frame(W, H, 0)
    dt = CDT[storage]
    src = np.concatenate([f["radiance"][..., :3], rng.uniform(0.0, 0.05, (H, W, 1)).astype(np.float32)], -1).astype(dt)
    gb = G.gb_dev(f)
    for step, phi_c, phi_n in [(32, 10.0, 128.0), (64, 10.0, 128.0), (512, 10.0, 128.0), (2, 10.0, 0.0), (16, 10.0, 0.0), (1, 0.0, 128.0), (4, 0.0, 0.0)]:
        want = np.zeros_like(src)
        oracle.atrous(W, H, storage, src, want, None, gbuf(f), step=step, phi_colour=phi_c, phi_normal=phi_n, iteration=1, nthreads=8)
        d = F.Denoiser(W, H, F.Params(storage=storage, phi_colour=phi_c, phi_normal=phi_n))
        out = d.new_colour()
        d.FilterKernel(G.dev(src), out, None, gb, step, 1)
        G.assert_colour_close(G.host(out), want, storage, f"step {step} phi_colour {phi_c} phi_normal {phi_n}")


@pytest.mark.parametrize("variant", ["auto", "direct", "lds-general"])
@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_moments_degenerate_phis(G, oracle, storage, variant):
    """The spatial estimate at the ends of the GUI's drags (src/GUI.cpp:991-992, both start at 0): PhiColour = 0 makes |dl| / PhiColour inf — or
    NaN where the tap's luminance IS the centre's, the centre tap included — and `max(., 0.0)` = fmax reads a NaN as no term (Filter.cuh:422-424):
    finite results.  (Found by tests/fuzz_parity.py: the streaming kernel's exact second evaluation was tied to a non-finite texel having been
    staged and wrote NaN for every young pixel.)  PhiNormal = 0: pow(x, 0) = 1 also at x = 0.  Stage call and frame driver (cold frames: the
    streaming kernel; steady state: the young-pixel launch)."""
    from svgf_amd import filter as F
    W, H = 203, 131
    rng = np.random.default_rng(9)
    f = synth.make_frame(W, H, 0)
    dt = CDT[storage]
    col = rng.uniform(0, 1, (H, W, 4)).astype(dt)
    col[40:60, 50:90, :3] = col[40, 50, :3]                   # a patch of equal luminance: its taps pass PhiColour = 0
    mom = rng.uniform(0, 1, (H, W, 2)).astype(dt)
    hist = rng.integers(1, 6, (H, W)).astype(np.uint8)
    for phi_c, phi_n in [(0.0, 128.0), (10.0, 0.0), (0.0, 0.0), (1e-6, 1e-3)]:
        want = np.zeros_like(col)
        oracle.moments(W, H, storage, col, want, mom, gbuf(f), hist, phi_colour=phi_c, phi_normal=phi_n, radius=3)
        assert np.isfinite(want.astype(np.float32)).all()
        d = F.Denoiser(W, H, F.Params(storage=storage, phi_colour=phi_c, phi_normal=phi_n, variant=variant))
        out = d.new_colour()
        d.FilterMoments(G.dev(col), out, G.dev(mom), G.gb_dev(f), G.dev(hist))
        got = G.host(out)
        assert np.isfinite(got.astype(np.float32)).all(), (phi_c, phi_n)
        if storage == "f32":
            assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 8e-5, (phi_c, phi_n)
        else:
            G.assert_colour_close(got[..., :3], want[..., :3], storage, f"moments phi {phi_c} {phi_n}")
        # the frame driver over the cold -> steady transition of a pan: finite, history equal to the oracle's
        fr = frames(W, H, 6, mv=(1.0, -1.5))
        ref = oracle.Pipeline(W, H, storage, steps=2, nthreads=8, phi_colour=phi_c, phi_normal=phi_n)
        dd = F.Denoiser(W, H, F.Params(storage=storage, steps=2, phi_colour=phi_c, phi_normal=phi_n, variant=variant))
        gbs = [G.gb_dev(x) for x in fr]
        for k in range(6):
            w = ref.frame(fr[k]["radiance"], gbuf(fr[k]), gbuf(fr[max(k - 1, 0)]))
            g = G.host(dd.Render(G.dev(fr[k]["radiance"].astype(G.NPDT[storage])), gbs[k], gbs[k - 1] if k else None))
            assert np.isfinite(g.astype(np.float32)).all() and np.isfinite(w.astype(np.float32)).all(), (phi_c, phi_n, k)
            assert np.array_equal(G.host(dd.state_plane(F.PLANE_HISTORY, 1 - dd.pingpong())), ref.taps["hist"]), (phi_c, phi_n, k)


def test_frame_sizes_and_ten_iterations(G, oracle):
    """Odd sizes around the 256-column / 64-lane tiles, narrower than one tile, and the GUI's maximum of 10 iterations."""
    for (W, H, steps) in [(1, 1, 2), (7, 3, 5), (17, 130, 5), (130, 2, 5), (64, 40, 3), (255, 33, 5), (257, 65, 5), (513, 130, 10)]:
        fr = frames(W, H, 3, mv=(1.0, 0.0))
        ref = oracle.Pipeline(W, H, "f32", steps=steps, nthreads=8)
        hip = G.HipPipeline(W, H, "f32", steps=steps)
        gbs = [G.gb_dev(f) for f in fr]
        for k in range(3):
            want = ref.frame(fr[k]["radiance"], gbuf(fr[k]), gbuf(fr[max(k - 1, 0)]))
            got = hip.frame(fr[k]["radiance"], gbs[k], gbs[max(k - 1, 0)])
            assert np.array_equal(hip.taps["hist"], ref.taps["hist"]), (W, H, k)
            G.assert_colour_close(got, want, "f32", f"{W}x{H} steps {steps} frame {k}")
        # the frame driver (fused launches, flags per 64-pixel segment) on the same sizes
        from svgf_amd import filter as F
        d = F.Denoiser(W, H, F.Params(storage="f32", steps=steps))
        ref2 = oracle.Pipeline(W, H, "f32", steps=steps, nthreads=8)
        for k in range(3):
            want = ref2.frame(fr[k]["radiance"], gbuf(fr[k]), gbuf(fr[max(k - 1, 0)]))
            got = G.host(d.Render(G.dev(fr[k]["radiance"]), gbs[k], gbs[k - 1] if k else None))
            assert np.array_equal(G.host(d.state_plane(F.PLANE_HISTORY, 1 - d.pingpong())), ref2.taps["hist"]), (W, H, k)
            assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 2e-3, (W, H, k)


def _look_at(eye, target, up=(0, 1, 0)):
    e, t, u = (np.asarray(v, np.float64) for v in (eye, target, up))
    f = t - e; f /= np.linalg.norm(f)
    s = np.cross(f, u); s /= np.linalg.norm(s)
    uu = np.cross(s, f)
    m = np.eye(4); m[0, :3], m[1, :3], m[2, :3] = s, uu, -f
    m[:3, 3] = -m[:3, :3] @ e
    return m


def _perspective(fovy, aspect, zn, zf):
    t = 1.0 / np.tan(fovy / 2)
    m = np.zeros((4, 4)); m[0, 0] = t / aspect; m[1, 1] = t; m[2, 2] = (zf + zn) / (zn - zf); m[2, 3] = 2 * zf * zn / (zn - zf); m[3, 2] = -1
    return m


def test_pack_gbuffer_adapter(G, oracle):
    """The stage in front of the path: GBuffer.frag texels from linear attribute planes, bit for
    bit against the C++ oracle (svgf_oracle_pack_gbuffer) and its NumPy twin, then fed to the temporal stage: a camera
    that does not move must reproject every covered pixel onto itself."""
    from oracle import svgf_numpy as snp
    from svgf_amd import filter as F
    W, H = 301, 187
    rng = np.random.default_rng(5)
    eye0, eye1 = np.array([0.3, 0.4, 5.0]), np.array([0.35, 0.38, 5.02])
    proj = _perspective(0.9, W / H, 0.1, 100.0)
    vp, pvp = proj @ _look_at(eye1, (0, 0, 0)), proj @ _look_at(eye0, (0, 0, 0))
    pos = np.concatenate([rng.uniform(-2, 2, (H, W, 3)), rng.integers(0, 900, (H, W, 1))], -1).astype(np.float32)
    nrm = np.concatenate([rng.normal(size=(H, W, 3)), rng.integers(0, 20, (H, W, 1))], -1).astype(np.float32)
    nrm[rng.uniform(size=(H, W)) < 0.1, :3] = 0                      # texels without geometry
    bary = np.concatenate([rng.uniform(0, 1, (H, W, 3)), rng.integers(0, 50, (H, W, 1))], -1).astype(np.float32)
    colmajor = lambda m: m.T.astype(np.float32).ravel()               # noqa: E731
    want_m, want_n, want_uv = oracle.pack_gbuffer(pos, nrm, bary, colmajor(vp), colmajor(pvp), eye1.astype(np.float32))
    for a_, b_ in zip((want_m, want_n, want_uv), snp.pack_gbuffer(pos, nrm, bary, colmajor(vp), colmajor(pvp), eye1.astype(np.float32))):
        assert np.array_equal(a_.view(np.uint8), b_.view(np.uint8)), "the two restatements of GBuffer.frag disagree"
    d = F.Denoiser(W, H, F.Params(storage="f32"))
    gb = d.PackGBuffer(G.dev(pos), G.dev(nrm), G.dev(bary), colmajor(vp), colmajor(pvp), eye1)
    got_m, got_n, got_uv = G.host(gb.motion), G.host(gb.normal).view(np.uint16), G.host(gb.uv).view(np.uint16)
    assert np.array_equal(got_m.view(np.uint32), want_m.view(np.uint32))
    assert np.array_equal(got_n, want_n) and np.array_equal(got_uv, want_uv)
    assert np.all(got_m[(nrm[..., :3] == 0).all(-1)] == 0)
    # static camera: zero motion on covered texels, and the filter accepts the reprojection everywhere but "sky"
    gb0 = d.PackGBuffer(G.dev(pos), G.dev(nrm), G.dev(bary), colmajor(vp), colmajor(vp), eye1)
    assert np.abs(G.host(gb0.motion)[..., :2]).max() == 0
    col, hist, mom = d.new_colour(), d.new_history(), d.new_moments()
    d.TemporalFilter(d.new_colour(), G.dev(rng.uniform(0, 1, (H, W, 4)).astype(np.float32)), col, gb0, gb0, G.dev(np.full((H, W), 5, np.uint8)),
                     hist, mom, d.new_moments())
    covered = ~(nrm[..., :3] == 0).all(-1)
    assert np.all(G.host(hist)[covered] == 6) and np.all(G.host(hist)[~covered] == 1)


@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_albedo_demodulation_bit_exact(G, oracle, storage):
    """svgf_demodulate / svgf_modulate (an extension, the reference has none) against the oracle, bit for bit
    (IEEE division), on a strip context too, in place, and the error paths."""
    from svgf_amd import filter as F
    rng = np.random.default_rng(78)
    W, H = 333, 77
    dt = CDT[storage]
    x = rng.uniform(0, 1, (H, W, 4)).astype(dt)
    alb = rng.uniform(-0.1, 1, (H, W, 4)).astype(dt)
    want_d = np.zeros_like(x); want_m = np.zeros_like(x)
    oracle.albedo(0, W, H, storage, x, alb, want_d)
    oracle.albedo(1, W, H, storage, want_d, alb, want_m)
    d = F.Denoiser(W, H, F.Params(storage=storage))
    xd, ad, od = G.dev(x), G.dev(alb), d.new_colour()
    d.Demodulate(xd, ad, od)
    assert np.array_equal(G.host(od).view(np.uint8), want_d.view(np.uint8))
    d.Modulate(od, ad, od)                                    # in place
    assert np.array_equal(G.host(od).view(np.uint8), want_m.view(np.uint8))
    ds = F.Denoiser(W, H, F.Params(storage=storage), strip=(16, 40, 24, 48))
    os_ = ds.new_colour()
    ds.Demodulate(G.dev(np.ascontiguousarray(x[16:56])), G.dev(np.ascontiguousarray(alb[16:56])), os_)
    assert np.array_equal(G.host(os_)[8:32].view(np.uint8), want_d[24:48].view(np.uint8))
    with pytest.raises(F.SvgfError, match="alias"):
        d.Demodulate(xd, ad, ad)
