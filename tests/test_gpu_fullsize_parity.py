"""GPU parity at the frame sizes the benchmark runs (1920x1080, 3840x2160) and at 7680x4320: each stage against the CPU oracle.

The launchers cut their work by the chip's CU count, so the streaming kernels run bands longer than the 8-row floor only on large frames
(tests/launch_geometry.py: 14-34 rows at 4K, 52-136 at 8K; every frame of test_gpu_parity.py and of the sweep's oracle kinds gets the floor).
Each test here first asks the geometry helper what the launch it checks looks like on THIS device and asserts that it is in the regime the
test claims to cover; then it fills the output planes with a NaN sentinel, runs the device, and compares with the oracle at the suite's stated
tolerances (tests/gpu_helpers.py:TOL) — bit for bit where the suite claims bit-exactness.

The planted texels: a NaN or a -0.0 own texel sends the band that holds it through atrous_band<..., true> again (svgf_atrous_lds.h).  A NaN
is put a few decimated rows before the END of some long bands, so that the rows a re-run must redo lie beyond the first eight."""
import gc
import os

import numpy as np
import pytest

from svgf_amd import synth
from tests import launch_geometry as LG
from tests.helpers import CDT, gbuf
from tests.plane_arena import SENTINEL, _is_sentinel, _sentinel_plane
from tests.test_gpu_nonfinite import assert_close_with_nan, assert_same_bits_or_nan

pytestmark = pytest.mark.gpu

NT = min(16, int(os.environ.get("OMP_NUM_THREADS") or 8))          # oracle threads (the GPU machines give a command 16 CPUs)
MIN_BAND = LG.constants()["kAtrousMinBand"]
PHI_C, PHI_N = 10.0, 128.0
PAN = (2.0, -3.0)


@pytest.fixture(scope="module")
def G():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tests import gpu_helpers
    return gpu_helpers


@pytest.fixture(scope="module")
def cus(G):
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


_FRAMES = {}


@pytest.fixture(scope="module")
def frames_of():
    """Synthetic frames by (W, H, scene, frame index, mv), made once per module (seconds each at 4K) and freed at its end."""
    def get(W, H, k=0, scene="planar", mv=(0.0, 0.0)):
        key = (W, H, k, scene, mv)
        if key not in _FRAMES:
            if W * H > 4096 * 2160:                                  # (an 8K frame: the others of that size first leave)
                for kk in [kk for kk in _FRAMES if kk[0] * kk[1] > 4096 * 2160]:
                    del _FRAMES[kk]
            _FRAMES[key] = synth.make_frame(W, H, k, scene=scene, mv=mv)
        return _FRAMES[key]
    yield get
    _FRAMES.clear()
    gc.collect()


def _band_of(ys, S, geo):
    """(row residue, band, decimated offset inside the band) of frame rows ys under the cut `geo` (atrous_lds_kernel)."""
    r, j = ys % S, ys // S
    return r, j // geo["band"], j % geo["band"]


def _where(bad, S, geo, n=6):
    """The first few pixels of a mask, with the band / tile they belong to: what a failure message names."""
    px = np.argwhere(bad.reshape(bad.shape[0], bad.shape[1], -1).any(-1))[:n]
    out = []
    for y, x in px:
        r, b, o = _band_of(np.int64(y), S, geo)
        out.append(f"(y {y} x {x}: residue {r} band {b} row {o} of {geo['band']}, x tile {x // 128})")
    return " ".join(out)


def _plant(rng, src, region, S, geo, with_blocks=True):
    """NaN texels and -0.0 blocks in a handful of bands, away from the frame's edges.  -> (the workgroup tiles that hold a planted texel, as
    (residue, band, x tile); how many NaNs sit at a band offset of MIN_BAND or more)."""
    H, W = region.shape
    m = 4 * S + 8
    surf = region != synth.SKY
    bands, late = set(), 0
    # one NaN (one channel) three decimated rows before the end of a few long bands in the middle of the frame
    nb, band = geo["nbands"], geo["band"]
    cand = list(range(1, nb - 1)) if nb > 2 else [0]
    for b in rng.choice(cand, size=min(4, len(cand)), replace=False):
        r = int(rng.integers(0, S))
        y = r + S * (int(b) * band + band - 3)
        if not (m <= y < H - m):
            continue
        xs = np.nonzero(surf[y, m:W - m])[0] + m
        if not len(xs):
            continue
        x = int(rng.choice(xs))
        src[y, x, int(rng.integers(0, 4))] = np.nan
        bands.add((r, int(b), x // 128)); late += 1
    # a few more anywhere inside, on surface and on sky texels
    for pool in (np.argwhere(surf[m:H - m, m:W - m]) + m, np.argwhere(~surf[m:H - m, m:W - m]) + m):
        if len(pool):
            for y, x in pool[rng.integers(0, len(pool), 4)]:
                src[y, x, int(rng.integers(0, 4))] = np.nan
                r, b, o = _band_of(y, S, geo)
                bands.add((int(r), int(b), int(x) // 128)); late += int(o >= MIN_BAND)
    if with_blocks:
        # -0.0 blocks: two on surfaces (24 x 48, a random subset of the channels), one on the sky (all channels)
        for pool, (h, w), all_ch in ((np.argwhere(surf[m:H - m - 24, m:W - m - 48]) + m, (24, 48), False),
                                     (np.argwhere(surf[m:H - m - 24, m:W - m - 48]) + m, (24, 48), False),
                                     (np.argwhere(~surf[m:H - m - 8, m:W - m - 64]) + m, (8, 64), True)):
            if not len(pool):
                continue
            y, x = pool[rng.integers(0, len(pool))]
            ch = [0, 1, 2, 3] if all_ch else (np.nonzero(rng.integers(0, 2, 4))[0].tolist() or [1])
            src[y:y + h, x:x + w, ch] = -0.0
            for yy in range(y, y + h):
                r, b, _ = _band_of(yy, S, geo)
                bands.update((int(r), int(b), xt) for xt in range(x // 128, (x + w - 1) // 128 + 1))
    return bands, late


def _atrous_case(G, oracle, fr, storage, S, geo, seed, with_blocks=True):
    """One a-trous stage call (iteration 0 with the feedback plane, iteration 1 without) against the oracle on a planted copy of the frame's
    radiance; everything test_gpu_parity.py:test_atrous asserts, plus the sentinel."""
    from svgf_amd import filter as F
    H, W = fr["region"].shape
    rng = np.random.default_rng(seed)
    dt = CDT[storage]
    src = np.concatenate([fr["radiance"][..., :3] * 1.2 - 0.05, rng.uniform(-0.01, 0.05, (H, W, 1)).astype(np.float32)], -1).astype(dt)
    bands, late = _plant(rng, src, fr["region"], S, geo, with_blocks)
    assert 0 < len(bands) < geo["tiles"] // 4, f"the planted texels must flag some bands and not their neighbours ({len(bands)} of {geo['tiles']} tiles)"
    want = np.zeros_like(src)
    oracle.atrous(W, H, storage, src, want, None, gbuf(fr), step=S, phi_colour=PHI_C, phi_normal=PHI_N, iteration=0, nthreads=NT)
    sky = fr["region"] == synth.SKY
    what = f"{W}x{H} {storage} step {S} (bands of {geo['band']} rows, {geo['nbands']} per residue, xgroup {geo['xgroup']})"

    d = F.Denoiser(W, H, F.Params(storage=storage, phi_colour=PHI_C, phi_normal=PHI_N, variant="auto"))
    gb = G.gb_dev(fr)
    src_d = G.dev(src)
    out, fb = _sentinel_plane((H, W, 4), storage), _sentinel_plane((H, W, 4), storage)
    d.FilterKernel(src_d, out, fb, gb, S, 0)
    got, got_fb = G.host(out), G.host(fb)
    unwritten = _is_sentinel(got, storage)
    assert not unwritten.any(), f"{what}: {unwritten.sum()} values never written: {_where(unwritten, S, geo)}"
    wn, gn = np.isnan(want.astype(np.float32)), np.isnan(got.astype(np.float32))
    assert np.array_equal(wn, gn), f"{what}: NaN masks differ at {_where(wn != gn, S, geo)}"
    assert_close_with_nan(G, got, want, storage, what)
    assert_same_bits_or_nan(got[sky], want[sky], what + ": sky copy")             # raw bits, the sign of a zero included
    zero = want == 0
    if S <= 4 and with_blocks:
        assert (np.signbit(want[zero]) & ~sky[..., None].repeat(4, -1)[zero]).sum() > 0, "the case holds no filtered -0.0"
    bad = zero & ~((got == 0) & (np.signbit(got) == np.signbit(want)))
    assert not bad.any(), f"{what}: the sign of a zero differs at {_where(bad, S, geo)}"
    assert _is_sentinel(got_fb[sky], storage).all(), what + ": feedback written on sky"
    assert np.array_equal(got_fb[~sky].view(np.uint8), got[~sky].view(np.uint8)), what + ": feedback differs from the output off sky"
    del got_fb, want
    # iteration != 0: no feedback, the same output
    out2, fb2 = _sentinel_plane((H, W, 4), storage), _sentinel_plane((H, W, 4), storage)
    d.FilterKernel(src_d, out2, fb2, gb, S, 1)
    assert _is_sentinel(G.host(fb2), storage).all(), what + ": iteration 1 wrote the feedback plane"
    assert np.array_equal(G.host(out2).view(np.uint8), got.view(np.uint8)), what + ": iteration 1 differs from iteration 0"
    d.close()
    return late


def _atrous_geo(W, H, S, cus, long=True):
    geo = LG.atrous_lds(W, H, S, cus)
    if long:
        assert geo["band"] > MIN_BAND, f"{W}x{H} step {S} on {cus} CUs: bands of {geo['band']} rows — not the long-band regime this test covers"
    assert geo["xgroup"] > 1, f"{W}x{H} step {S} on {cus} CUs: xgroup {geo['xgroup']}"
    return geo


# ------------------------------------------------------------------ a. 3840x2160
@pytest.mark.parametrize("step", [1, 2, 4, 8, 16, 32, 64])
@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_atrous_4k_planar(G, oracle, cus, frames_of, storage, step):
    """The product path (variant auto) at BASELINE's size on the headline planar scene, where most waves take the uniform-normal taps:
    14-row bands at steps 1-8, 18 (last band 9) at 16, 24 at 32, one 34-row band per residue at 64."""
    W, H = 3840, 2160
    geo = _atrous_geo(W, H, step, cus)
    if step <= 2:
        assert geo["padding"] > 0, f"step {step}: no padding workgroups ({geo})"
    late = _atrous_case(G, oracle, frames_of(W, H), storage, step, geo, seed=41 + step)
    assert late > 0, "no planted NaN lies beyond the first rows of its band"


@pytest.mark.parametrize("step", [1, 4, 16])
def test_atrous_4k_curved(G, oracle, cus, frames_of, step):
    """The general tap path: every surface texel of the curved scene has a normal of its own."""
    W, H = 3840, 2160
    geo = _atrous_geo(W, H, step, cus)
    assert _atrous_case(G, oracle, frames_of(W, H, scene="curved"), "f32", step, geo, seed=61 + step) > 0


# ------------------------------------------------------------------ b. 1920x1080
@pytest.mark.parametrize("step", [1, 2, 4, 8, 16])
@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_atrous_1080p(G, oracle, cus, frames_of, storage, step):
    """BASELINE configs[1] and `bench.py --full`'s 1080p leg: the bands are at the floor here, the tile groups and padding are this size's."""
    W, H = 1920, 1080
    geo = _atrous_geo(W, H, step, cus, long=False)
    assert geo["band"] == MIN_BAND, geo
    _atrous_case(G, oracle, frames_of(W, H), storage, step, geo, seed=81 + step)


# ------------------------------------------------------------------ d, e. 3840x2160 under a pan
def _seq(frames_of, N=5):
    return [frames_of(3840, 2160, k, mv=PAN) for k in range(N)]


@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_pipeline_stagewise_4k(G, oracle, cus, frames_of, storage):
    """test_gpu_parity.py:test_pipeline_stagewise_identical_inputs at full size: five frames of a pan, variant auto, every device stage fed the
    oracle's own inputs.  The moments stage call runs moments_lds_kernel (16-row bands) on every frame: every pixel is young in frames 0-2,
    only the disoccluded ones later.  Temporal colour, moments and history bit-exact; the moments estimate and all five a-trous iterations of
    every frame within the stage tolerances."""
    from svgf_amd import filter as F
    W, H, N = 3840, 2160, 5
    mg = LG.moments_lds(W, H, cus)
    assert mg["band"] > MIN_BAND, f"moments_lds_kernel: bands of {mg['band']} rows on {cus} CUs"
    geos = {1 << i: _atrous_geo(W, H, 1 << i, cus) for i in range(5)}
    fr = _seq(frames_of, N)
    ref = oracle.Pipeline(W, H, storage, steps=5, nthreads=NT)
    d = F.Denoiser(W, H, F.Params(storage=storage, steps=5, variant="auto"))
    gbs = [G.gb_dev(f) for f in fr]
    young_later = 0
    for k in range(N):
        kp = max(k - 1, 0)
        ref.frame(fr[k]["radiance"], gbuf(fr[k]), gbuf(fr[kp]))
        t = ref.taps
        if k >= 3:
            young_later = int((t["hist"] < 4).sum())
            assert 0 < young_later < W * H // 4, f"frame {k}: {young_later} young pixels"
        col, mom = _sentinel_plane((H, W, 4), storage), _sentinel_plane((H, W, 2), storage)
        hist = d.new_history(); hist.fill_(255)
        d.TemporalFilter(G.dev(t["prev_colour"]), G.dev(t["radiance"]), col, gbs[k], gbs[kp], G.dev(t["prev_hist"]), hist, mom, G.dev(t["prev_mom"]))
        assert np.array_equal(G.host(hist), t["hist"]), f"frame {k}: history mask mismatch"
        assert np.array_equal(G.host(col).view(np.uint8), t["temporal"].view(np.uint8)), f"frame {k}: temporal colour"
        assert np.array_equal(G.host(mom).view(np.uint8), t["mom"].view(np.uint8)), f"frame {k}: temporal moments"
        out = _sentinel_plane((H, W, 4), storage)
        d.FilterMoments(G.dev(t["temporal"]), out, G.dev(t["mom"]), gbs[k], G.dev(t["hist"]))
        got, want = G.host(out), t["moments"]
        assert not _is_sentinel(got, storage).any(), f"frame {k}: moments output not written everywhere"
        lim = 8e-5 if storage == "f32" else 1e-3                         # test_pipeline_stagewise_identical_inputs' bounds
        assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= lim, f"frame {k}: moments"
        sky = fr[k]["region"] == synth.SKY
        for i in range(5):
            fb = G.dev(t["temporal"]) if i == 0 else None
            out = _sentinel_plane((H, W, 4), storage)
            d.FilterKernel(G.dev(t["atrous_in"][i]), out, fb, gbs[k], 1 << i, i)
            got = G.host(out)
            assert not _is_sentinel(got, storage).any(), f"frame {k} a-trous iteration {i}: unwritten at {_where(_is_sentinel(got, storage), 1 << i, geos[1 << i])}"
            G.assert_colour_close(got, t["atrous_out"][i], storage, f"frame {k} a-trous iteration {i}")
            if i == 0:
                assert np.array_equal(G.host(fb).view(np.uint8)[sky], t["temporal"].view(np.uint8)[sky])
    d.close()
    assert young_later > 0


@pytest.mark.parametrize("prev_guide", [False, True])
@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_frame_driver_4k_pan_equals_stage_calls(G, cus, frames_of, storage, prev_guide):
    """svgf_denoise_frame in the benchmark's configuration (variant auto, iterations 0 + 1 as one launch: 68-row bands; svgf_set_prev_guide
    off and on) against the plain stage calls on caller-owned planes, bit for bit, over the same pan.  From frame 3 on the driver serves
    the young pixels with the young-pixel launch where the stage call runs the streaming moments kernel.  With
    test_pipeline_stagewise_4k this ties the frame driver to the oracle at 4K."""
    import torch
    from svgf_amd import filter as F
    W, H, N = 3840, 2160, 5
    pg = LG.atrous_fused12(W, H, cus)
    assert pg["band"] > 32 and pg["xgroup"] > 1, f"atrous_fused12_kernel on {cus} CUs: {pg}"
    assert LG.moments_lds(W, H, cus)["band"] > MIN_BAND
    yl = LG.young_launch(W, H, cus)
    assert yl["scan"] > 0 and yl["walk"] > 0 and yl["cap"] >= 1024
    for S in (4, 8, 16):
        _atrous_geo(W, H, S, cus)
    fr = _seq(frames_of, N)
    gbs = [G.gb_dev(f) for f in fr]
    hip = G.HipPipeline(W, H, storage, steps=5, variant="auto")
    d = F.Denoiser(W, H, F.Params(storage=storage, steps=5, variant="auto"))
    d.set_iteration_fusion(True)
    d.set_prev_guide(prev_guide)
    u, v = SENTINEL[storage]
    for k in range(N):
        kp = max(k - 1, 0)
        for plane in (hip.colour[hip.P], hip.filt[0], hip.filt[1]):
            plane.copy_(_sentinel_plane(tuple(plane.shape), storage))
        rad = fr[k]["radiance"]
        want = hip.frame(rad, gbs[k], gbs[kp])
        assert not _is_sentinel(want, storage).any() and not _is_sentinel(hip.taps["moments"], storage).any(), f"frame {k}: stage calls left texels unwritten"
        got = d.Render(G.dev(rad.astype(G.NPDT[storage])), gbs[k], gbs[kp] if k else None)
        torch.cuda.synchronize()
        assert np.array_equal(G.host(got).view(np.uint8), want.view(np.uint8)), f"frame {k}"
        assert np.array_equal(G.host(d.state_plane(F.PLANE_HISTORY, 1 - d.pingpong())), hip.taps["hist"]), f"frame {k}: history"
        assert np.array_equal(G.host(d.state_plane(F.PLANE_MOMENTS, 1 - d.pingpong())).view(np.uint8), hip.taps["mom"].view(np.uint8)), f"frame {k}: moments"
    assert int((hip.taps["hist"] < 4).sum()) > 0, "the pan left no young pixel for the young-pixel launch"
    d.close()


# ------------------------------------------------------------------ c. 7680x4320
@pytest.mark.parametrize("step", [1, 16])
def test_atrous_8k(G, oracle, cus, frames_of, step):
    """The only size at which bands of about 52 rows exist today (52 at step 1, 68 at step 16), with planted NaN and -0.0 texels."""
    W, H = 7680, 4320
    geo = _atrous_geo(W, H, step, cus)
    assert geo["band"] >= 52, geo
    assert _atrous_case(G, oracle, frames_of(W, H), "f32", step, geo, seed=101 + step) > 0
