"""Every stage call with ALL its planes inside one caller arena (tests/plane_arena.py): what the kernels touch outside their planes.

Each case runs under the three margin fills ("nan", "zero", "live") in the spaced layout and once in the tight layout (planes back to
back, live margins at the arena's ends), every plane at a base that is 0, 1 or 3 texels behind a 512-byte boundary, and asserts
  1. fill independence: the output planes hold the same bits under all four (a NaN's payload is not compared);
  2. parity of one of them with the oracle at the suite's existing claims (tests/gpu_helpers.py:TOL; bit for bit where that is claimed);
  3. every margin byte and every input plane as they were (the documented aliases are outputs);
  4. the write set: outputs start as the sentinel; what the contract says is written is not the sentinel, what it says is not written still is.

Alignment, by reading the kernels (include/svgf.h, Conventions): no load or store is wider than the texel it addresses — colour b128 / b64,
{depth, ddepth} b64 at +8 of the 16-byte motion texel, normal / uv b64, moments b64 / b32, history b8 (svgf_device.h: Store<>, raw_load;
svgf_moments_lds.h; svgf_atrous_lds.h / svgf_atrous_fused.h stores) — so a texel-aligned base keeps every access naturally aligned, as a
ragged width already does for every row.  No entry point needs to refuse a pointer.

Which "live" case sees what (for a reviewer who lengthens a num_records by a row, or drops an in-frame test, in a scratch copy):
  a-trous, streaming  test_atrous[lds-*]: the taps of the first / last 2 * step rows read the mirrored rows at full weight (same surface);
  a-trous, direct     test_atrous[direct-*] likewise through `py < 0 || py >= g.H`;
  moments             test_moments[*]: rows 0-2 and H-3..H-1 of the young pixels (hist < 4 everywhere near the edges);
  temporal            test_temporal[edge-rows]: the first / last rows reproject 3 rows out of the frame onto the mirrored previous planes, which
                      pass the depth / normal / ID tests (same surface) — history and colour would accumulate instead of resetting;
  TAA                 test_taa: row 0 samples row -1..-3 without the clamp of tex_coord;
  adapter             test_pack_gbuffer: the quad partner of the last row / column (H, W odd);
  strips              test_strip_contexts: a reprojection that lands inside the frame but outside the strip reads the mirrored previous planes
                      without the strip guard and is accepted (history != 1, fewer violations than the host counts); a tap row indexed by its
                      frame row instead of its strip row leaves the plane.  The strip holds exactly the 2 * step halo of its owned rows (check_halo
                      refuses less), so no tap of an owned row has a strip row of -1 or `rows`: the strip half of `row_ok` only keeps rows that a
                      band stages beyond the halo, and that no owned pixel uses, off the neighbouring plane — an off-by-one THERE changes no
                      value and is beyond what a test of values can see; the frame half (`y < H`) is test_atrous[lds-*]'s."""
import ctypes as C

import numpy as np
import pytest

from svgf_amd import synth
from tests import plane_arena as PA
from tests.helpers import CDT, gbuf, half_ulp_diff

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (63, 5), (65, 9), (129, 40), (331, 203), (640, 37)]
FULL = (331, 203)                                    # the size that carries the cross products
LAYOUTS = [("nan", False), ("zero", False), ("live", False), ("live", True)]
PHI_C, PHI_N = 10.0, 128.0


@pytest.fixture(scope="module")
def G():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tests import gpu_helpers
    return gpu_helpers


def _same_bits(a, b):
    if a.dtype.kind != "f":
        return np.array_equal(a.view(np.uint8), b.view(np.uint8))
    na, nb = np.isnan(a.astype(np.float32)), np.isnan(b.astype(np.float32))
    u = {2: np.uint16, 4: np.uint32}[a.dtype.itemsize]
    return np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb])


def in_arenas(specs, inputs, call, *, margin_rows, what, prefill=None, like=None):
    """Run call(arena) under every layout.  inputs: name -> host array (checked intact); prefill: name -> what an output starts as (default: the
    sentinel).  -> (outputs of the first layout: name -> host array, what call() returned there)."""
    import torch
    runs = []
    for li, (fill, tight) in enumerate(LAYOUTS):
        offs = {name: PA.OFFSETS[(i + li) % 3] for i, (name, _, _) in enumerate(specs)}
        ar = PA.Arena(specs, {**inputs, **(prefill or {})}, fill=fill, tight=tight, margin_rows=margin_rows, offsets=offs, like=like, seed=li)
        ar.snapshot_inputs(*inputs)
        extra = call(ar)
        torch.cuda.synchronize()
        tag = f"{what} [{fill}{', tight' if tight else ''}]"
        ar.check(tag)
        runs.append((tag, {n: ar.host(n) for n, _, _ in specs if n not in inputs}, extra))
    tag0, out0, extra0 = runs[0]
    for tag, out, extra in runs[1:]:
        for n in out0:
            assert _same_bits(out[n], out0[n]), f"{tag}: plane '{n}' differs from {tag0}: the result depends on what lies around the planes"
        assert extra == extra0, f"{tag}: {extra} against {extra0}"
    return out0, extra0


def _gb_specs(H, W, pre=""):
    return [(pre + "motion", (H, W, 4), np.float32), (pre + "normal", (H, W, 4), np.uint16), (pre + "uv", (H, W, 4), np.uint16)]


def _gb_of(F, ar, pre=""):
    return F.GBuffer(ar.view(pre + "motion"), ar.view(pre + "normal"), ar.view(pre + "uv"))


def _gb_in(f, pre=""):
    return {pre + k: f[k] for k in ("motion", "normal", "uv")}


def _written(a):
    return ~PA.is_sentinel_array(a)


# ------------------------------------------------------------------ temporal
MOTIONS = {"static": 0, "pan": 2, "edge-rows": 3, "wrap": 8}


def _temporal_inputs(W, H, storage, motion, seed=1):
    rng = np.random.default_rng(seed)
    dt = CDT[storage]
    mv = (-2.5, 1.5) if motion == "pan" else (0.0, 0.0)
    f0, f1 = synth.make_frame(W, H, 3, mv=mv), synth.make_frame(W, H, 4, mv=mv)
    f1 = dict(f1)
    f1["motion"] = f1["motion"].copy()
    if motion == "edge-rows":                        # the upper half reprojects 3 rows up, the lower half 3 rows down: rows 0-2 and H-3.. leave the frame
        f1["motion"][: (H + 1) // 2, :, 1] = -3.0
        f1["motion"][(H + 1) // 2:, :, 1] = 3.0
        f1["motion"][..., 0] = 0.0
    if motion == "wrap":                             # cvt.rzi saturates; x + INT_MAX wraps to a negative coordinate (svgf_device.h: add_wrap)
        vals = np.array([3e9, -3e9, 2147483520.0, -2147483648.0, np.inf, -np.inf, np.nan, 4294967296.0], np.float32)
        f1["motion"][..., 0] = vals[np.arange(W) % len(vals)][None, :]
        f1["motion"][..., 1] = vals[(np.arange(H) * 3 + 1) % len(vals)][:, None]
    prev = rng.uniform(-0.1, 1.2, (H, W, 4)).astype(dt)
    mom_prev = rng.uniform(0, 1, (H, W, 2)).astype(dt)
    hist_prev = rng.integers(0, 40, (H, W)).astype(np.uint8)
    cur = (f1["radiance"] * 1.3 - 0.1).astype(dt)
    return f0, f1, prev, mom_prev, hist_prev, cur


def _temporal_case(G, oracle, W, H, storage, motion, mesh, alias):
    from svgf_amd import filter as F
    dt = CDT[storage]
    f0, f1, prev, mom_prev, hist_prev, cur = _temporal_inputs(W, H, storage, motion)
    out = np.zeros_like(cur); hist = np.zeros((H, W), np.uint8); mom = np.zeros((H, W, 2), dt)
    oracle.temporal(W, H, storage, prev, cur, out, gbuf(f1), gbuf(f0), hist_prev, hist, mom, mom_prev,
                    depth_threshold=0.8, normal_threshold=0.9, history_base=24, mesh_id_test=mesh)
    if motion == "edge-rows" and H >= 8 and (f1["motion"][..., 2] != 0).any():
        edge = np.r_[0:3, H - 3:H]
        assert (hist[edge] == 1).all(), "the rows that reproject out of the frame must reset their history"
    specs = _gb_specs(H, W, "c_") + _gb_specs(H, W, "p_") + [("prev", (H, W, 4), dt), ("colour", (H, W, 4), dt), ("mom_prev", (H, W, 2), dt),
             ("mom", (H, W, 2), dt), ("hist_prev", (H, W), np.uint8), ("hist", (H, W), np.uint8)]
    inputs = {**_gb_in(f1, "c_"), **_gb_in(f0, "p_"), "prev": prev, "mom_prev": mom_prev, "hist_prev": hist_prev}
    prefill, like = {}, {"mom": "mom_prev", "hist": "hist_prev"}
    if alias:                                        # radiance == colour_out: the reference's in-place CurrentImage (svgf.h)
        prefill["colour"] = cur
    else:
        specs.append(("radiance", (H, W, 4), dt)); inputs["radiance"] = cur; like["colour"] = "prev"
    d = F.Denoiser(W, H, F.Params(storage=storage, mesh_id_test=mesh))

    def call(ar):
        d.TemporalFilter(ar.view("prev"), ar.view("colour" if alias else "radiance"), ar.view("colour"), _gb_of(F, ar, "c_"), _gb_of(F, ar, "p_"),
                         ar.view("hist_prev"), ar.view("hist"), ar.view("mom"), ar.view("mom_prev"))
    what = f"temporal {W}x{H} {storage} {motion} mesh {mesh}{' in place' if alias else ''}"
    got, _ = in_arenas(specs, inputs, call, margin_rows=MOTIONS[motion] + 8, what=what, prefill=prefill, like=like)
    d.close()
    assert np.array_equal(got["hist"], hist), what + ": history"
    assert _same_bits(got["colour"], out), what + ": colour"
    assert _same_bits(got["mom"], mom), what + ": moments"
    # the write set: every texel of the three outputs (the oracle's values are no sentinel; a NaN result would be one of the input's)
    assert _written(got["mom"]).all() and (alias or _written(got["colour"]).all()), what + ": a texel was not written"
    assert (got["hist"] != PA.BYTE_SENTINEL).all(), what + ": a history texel was not written"


@pytest.mark.parametrize("alias", [False, True])
@pytest.mark.parametrize("mesh", [0, 1])
@pytest.mark.parametrize("motion", list(MOTIONS))
@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_temporal(G, oracle, storage, motion, mesh, alias):
    _temporal_case(G, oracle, *FULL, storage, motion, mesh, alias)


@pytest.mark.parametrize("size", [s for s in SIZES if s != FULL])
@pytest.mark.parametrize("motion", ["pan", "edge-rows"])
@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_temporal_sizes(G, oracle, storage, motion, size):
    _temporal_case(G, oracle, *size, storage, motion, 1, False)


# ------------------------------------------------------------------ moments
def _moments_parity(G, got, want, col, hist, storage, what, stagewise=False):
    keep = hist >= 4
    assert np.array_equal(got[keep].view(np.uint8), col[keep].view(np.uint8)), what + ": copied texels"
    if stagewise:                                    # test_gpu_parity.py:test_pipeline_stagewise_identical_inputs' bounds (the temporal stage's output as input)
        assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= (8e-5 if storage == "f32" else 1e-3), what
    elif storage == "f32":                             # test_gpu_parity.py:test_moments' bounds
        g, w = got.astype(np.float64), want.astype(np.float64)
        assert np.abs(g[..., :3] - w[..., :3]).max() <= 2e-5, what
        assert np.abs(g[..., 3] - w[..., 3]).max() <= 2e-5 * 4, what
    else:
        G.assert_colour_close(got[..., :3], want[..., :3], storage, what)
        g, w = got[..., 3].astype(np.float64), want[..., 3].astype(np.float64)
        assert np.all(np.abs(g - w) <= 8e-5 + np.abs(w) * 2.0 ** -10), what


def _moments_case(G, oracle, W, H, storage, radius, variant):
    from svgf_amd import filter as F
    rng = np.random.default_rng(2)
    dt = CDT[storage]
    f = synth.make_frame(W, H, 0)
    col = rng.uniform(0, 1, (H, W, 4)).astype(dt)
    mom = rng.uniform(0, 1, (H, W, 2)).astype(dt)
    hist = rng.integers(1, 8, (H, W)).astype(np.uint8)
    hist[:4] = np.minimum(hist[:4], 3); hist[-4:] = np.minimum(hist[-4:], 3)      # the rows whose windows reach the margins are young
    want = np.zeros_like(col)
    oracle.moments(W, H, storage, col, want, mom, gbuf(f), hist, phi_colour=PHI_C, phi_normal=PHI_N, radius=radius)
    specs = _gb_specs(H, W)[:2] + [("colour", (H, W, 4), dt), ("out", (H, W, 4), dt), ("mom", (H, W, 2), dt), ("hist", (H, W), np.uint8)]
    inputs = {"motion": f["motion"], "normal": f["normal"], "colour": col, "mom": mom, "hist": hist}
    d = F.Denoiser(W, H, F.Params(storage=storage, moments_radius=radius, variant=variant, phi_colour=PHI_C, phi_normal=PHI_N))

    def call(ar):
        gb = F.GBuffer(ar.view("motion"), ar.view("normal"), None)
        d.FilterMoments(ar.view("colour"), ar.view("out"), ar.view("mom"), gb, ar.view("hist"))
    what = f"moments {W}x{H} {storage} radius {radius} {variant}"
    got, _ = in_arenas(specs, inputs, call, margin_rows=3 + 8, what=what, like={"out": "colour"})
    d.close()
    assert _written(got["out"]).all(), what + ": a texel was not written"
    _moments_parity(G, got["out"], want, col, hist, storage, what)


@pytest.mark.parametrize("radius,variant", [(3, "direct"), (3, "lds"), (3, "auto"), (3, "lds-general"), (1, "auto"), (1, "direct")])
@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_moments(G, oracle, storage, radius, variant):
    """radius 3: moments_pixel (direct) and moments_lds_kernel; radius 1: moments3x3_shfl_kernel (its edge lanes fetch the column beyond the wave)
    and its direct twin."""
    _moments_case(G, oracle, *FULL, storage, radius, variant)


@pytest.mark.parametrize("size", [s for s in SIZES if s != FULL])
@pytest.mark.parametrize("radius,variant", [(3, "auto"), (3, "direct"), (1, "auto")])
@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_moments_sizes(G, oracle, storage, radius, variant, size):
    _moments_case(G, oracle, *size, storage, radius, variant)


@pytest.mark.parametrize("feedback_follows", [False, True])
@pytest.mark.parametrize("variant", ["auto", "direct"])
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_temporal_moments(G, oracle, storage, size, variant, feedback_follows):
    """svgf_temporal_moments: the temporal launch's pass-through store and the young-pixel launch (moments_young_kernel: eight lanes per pixel,
    window taps clamped to the strip, the colour of an old tap read from filter_out).  filter_out == colour_out is refused and writes nothing."""
    from svgf_amd import filter as F
    W, H = size
    dt = CDT[storage]
    f0, f1, prev, mom_prev, hist_prev, cur = _temporal_inputs(W, H, storage, "pan")
    tcol = np.zeros_like(cur); hist = np.zeros((H, W), np.uint8); mom = np.zeros((H, W, 2), dt)
    oracle.temporal(W, H, storage, prev, cur, tcol, gbuf(f1), gbuf(f0), hist_prev, hist, mom, mom_prev,
                    depth_threshold=0.8, normal_threshold=0.9, history_base=24, mesh_id_test=1)
    want = np.zeros_like(cur)
    oracle.moments(W, H, storage, tcol, want, mom, gbuf(f1), hist, phi_colour=PHI_C, phi_normal=PHI_N, radius=3)
    # the young-pixel launch has work at every size; from 65x9 on old pixels sit among the young (1x1 and 63x5: every pixel is young)
    assert (hist < 4).any() and (H < 9 or (hist >= 4).any())
    specs = _gb_specs(H, W, "c_") + _gb_specs(H, W, "p_") + [("prev", (H, W, 4), dt), ("radiance", (H, W, 4), dt), ("colour", (H, W, 4), dt),
             ("filt", (H, W, 4), dt), ("mom_prev", (H, W, 2), dt), ("mom", (H, W, 2), dt), ("hist_prev", (H, W), np.uint8), ("hist", (H, W), np.uint8)]
    inputs = {**_gb_in(f1, "c_"), **_gb_in(f0, "p_"), "prev": prev, "radiance": cur, "mom_prev": mom_prev, "hist_prev": hist_prev}
    like = {"mom": "mom_prev", "hist": "hist_prev", "colour": "prev", "filt": "prev"}
    d = F.Denoiser(W, H, F.Params(storage=storage, variant=variant, phi_colour=PHI_C, phi_normal=PHI_N))

    def call(ar):
        d.TemporalMoments(ar.view("prev"), ar.view("radiance"), ar.view("colour"), ar.view("filt"), _gb_of(F, ar, "c_"), _gb_of(F, ar, "p_"),
                          ar.view("hist_prev"), ar.view("hist"), ar.view("mom"), ar.view("mom_prev"), feedback_follows=feedback_follows)
    what = f"temporal+moments {W}x{H} {storage} {variant} feedback_follows {feedback_follows}"
    got, _ = in_arenas(specs, inputs, call, margin_rows=3 + 2 + 8, what=what, like=like)
    assert np.array_equal(got["hist"], hist) and _same_bits(got["mom"], mom), what
    # colour_out: stored unless feedback_follows and iteration 0's feedback will overwrite it (history >= 4 on a texel with depth)
    z = f1["motion"][..., 2]
    skipped = feedback_follows & (hist >= 4) & (z != 0) & (z != np.float32(1e30))
    assert PA.is_sentinel_array(got["colour"])[skipped].all(), what + ": a colour_out texel that feedback overwrites was stored"
    assert _same_bits(got["colour"][~skipped], tcol[~skipped]), what + ": colour_out"
    assert _written(got["filt"]).all(), what + ": filter_out not written everywhere"
    _moments_parity(G, got["filt"], want, tcol, hist, storage, what, stagewise=True)

    def refused(ar):
        with pytest.raises(F.SvgfError, match="filter_out"):
            d.TemporalMoments(ar.view("prev"), ar.view("radiance"), ar.view("colour"), ar.view("colour"), _gb_of(F, ar, "c_"), _gb_of(F, ar, "p_"),
                              ar.view("hist_prev"), ar.view("hist"), ar.view("mom"), ar.view("mom_prev"))
    got, _ = in_arenas(specs, inputs, refused, margin_rows=8, what=what + " refused", like=like)
    assert all(PA.is_sentinel_array(v).all() for v in got.values()), "a refused call wrote a plane"
    d.close()


# ------------------------------------------------------------------ a-trous
def _atrous_src(rng, f, storage):
    H, W = f["region"].shape
    src = np.concatenate([f["radiance"][..., :3] * 1.2 - 0.05, rng.uniform(-0.01, 0.05, (H, W, 1)).astype(np.float32)], -1).astype(CDT[storage])
    # a NaN texel and a -0.0 block next to the first and the last rows: the exact second pass of those bands runs against the margins
    for y in {0, min(1, H - 1), H - 1, max(H - 2, 0)}:
        src[y, (7 * (y + 1)) % W, y % 4] = np.nan
    src[: min(3, H), W // 3: W // 3 + 9, 1] = -0.0
    src[max(H - 3, 0):, W // 2: W // 2 + 9] = -0.0
    return src


def _atrous_case(G, oracle, W, H, storage, variant, step, phi_n=PHI_N):
    from svgf_amd import filter as F
    from tests.test_gpu_nonfinite import assert_close_with_nan
    rng = np.random.default_rng(3 + step)
    dt = CDT[storage]
    f = synth.make_frame(W, H, 0)
    src = _atrous_src(rng, f, storage)
    want = np.zeros_like(src)
    oracle.atrous(W, H, storage, src, want, None, gbuf(f), step=step, phi_colour=PHI_C, phi_normal=phi_n, iteration=0)
    z = f["motion"][..., 2]
    sky = (z == 0) | (z == np.float32(1e30))
    specs = _gb_specs(H, W)[:2] + [("src", (H, W, 4), dt), ("out", (H, W, 4), dt), ("fb", (H, W, 4), dt)]
    inputs = {"motion": f["motion"], "normal": f["normal"], "src": src}
    d = F.Denoiser(W, H, F.Params(storage=storage, variant=variant, phi_colour=PHI_C, phi_normal=phi_n))
    streaming = variant != "direct" and step in (1, 2, 4, 8, 16, 32, 64) and phi_n != 0.0
    d.path_stats_enable(True)
    for feedback, iteration in ((True, 0), (False, 0), (True, 1), (False, 1)):
        def call(ar):
            gb = F.GBuffer(ar.view("motion"), ar.view("normal"), None)
            d.FilterKernel(ar.view("src"), ar.view("out"), ar.view("fb") if feedback else None, gb, step, iteration)
            return d.path_stats_read().get(step, (0, 0))[0] > 0
        what = f"a-trous {W}x{H} {storage} {variant} step {step} phi_normal {phi_n} feedback {feedback} iteration {iteration}"
        got, served_lds = in_arenas(specs, inputs, call, margin_rows=2 * step + 8, what=what, like={"out": "src", "fb": "src"})
        # which kernel served the call: the streaming kernel counts the wave-steps that filtered a surface pixel, the direct kernel counts nothing
        assert served_lds == (streaming and bool((~sky).any())), what + f": served by the {'streaming' if served_lds else 'direct'} kernel"
        out, fb = got["out"], got["fb"]
        assert _written(out).all(), what + ": an output texel was not written"
        assert_close_with_nan(G, out, want, storage, what)
        assert _same_bits(out[sky], want[sky]), what + ": sky copy"
        zero = want == 0
        assert np.array_equal(out[zero] == 0, want[zero] == 0) and np.array_equal(np.signbit(out[zero]), np.signbit(want[zero])), what + ": sign of zero"
        if feedback and iteration == 0:              # RenderOutput: non-sky texels only (svgf.h)
            assert PA.is_sentinel_array(fb)[sky].all(), what + ": feedback written on sky"
            assert _same_bits(fb[~sky], out[~sky]), what + ": feedback differs from the output"
        else:
            assert PA.is_sentinel_array(fb).all(), what + ": the feedback plane was written"
    d.close()


ATROUS = [(v, s) for v in ("lds", "lds-general") for s in (1, 2, 4, 8, 16, 32, 64)] + [("direct", s) for s in (1, 3, 5, 64)]


@pytest.mark.parametrize("variant,step", ATROUS, ids=[f"{v}-{s}" for v, s in ATROUS])
@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_atrous(G, oracle, storage, variant, step):
    """331 columns are narrower than the 128 + 4 S staging width from step 64 on; each case with and without the feedback plane, on iteration 0
    and on a later one."""
    _atrous_case(G, oracle, *FULL, storage, variant, step)


@pytest.mark.parametrize("size", [s for s in SIZES if s != FULL])
@pytest.mark.parametrize("variant,step", [("lds", 1), ("lds", 8), ("lds", 64), ("lds-general", 16), ("direct", 5)])
@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_atrous_sizes(G, oracle, storage, variant, step, size):
    """Frames shorter than the step (every size here at step 64, most at 8 and 16) and narrower than the staging width."""
    _atrous_case(G, oracle, *size, storage, variant, step)


@pytest.mark.parametrize("variant,step", [("auto", 1), ("lds", 4), ("direct", 16)])
@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_atrous_phi_normal_zero(G, oracle, storage, variant, step):
    """PhiNormal = 0 is the direct kernel's whatever the variant (launch_atrous)."""
    _atrous_case(G, oracle, *FULL, storage, variant, step, phi_n=0.0)


@pytest.mark.parametrize("size,rows", [(FULL, None), (FULL, (20, 150)), (FULL, (0, 7)), ((129, 40), None), ((640, 37), (6, 30)), ((65, 9), None), ((63, 5), None), ((1, 1), None)])
@pytest.mark.parametrize("variant", ["auto", "lds-general"])
@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_atrous_pair(G, oracle, storage, variant, size, rows):
    """svgf_atrous_pair (svgf_ext.h): `out` on the launch rows = what two svgf_atrous calls leave, bit for bit, and within the stage tolerance of
    the oracle's iteration 1 of that iteration 0; `feedback` on those rows and the 4 rows beyond them inside the frame, off the sky; nothing else.
    Then the same with a NaN texel and -0.0 blocks next to the first and last rows: the pair launch takes the exact form for every pixel of a band
    that holds such a texel, the two launches only for the pixels whose fast result does — the same values up to the rounding of iteration 0, which
    iteration 1's weights amplify; held to the bound of tests/fuzz_parity.py:trial_pair (2e-4 x max(1, 50 / PhiColour) fp32, 2e-2 fp16, NaN masks
    identical to the two launches' and to the oracle's), the feedback to the oracle at the stage tolerance.  Either way the sky texels are copies
    and a zero has the oracle's sign."""
    import torch
    from svgf_amd import filter as F
    from tests.test_gpu_nonfinite import assert_close_with_nan
    W, H = size
    dt = CDT[storage]
    f = synth.make_frame(W, H, 0)
    z = f["motion"][..., 2]
    sky = (z == 0) | (z == np.float32(1e30))
    rb, re = rows or (0, H)
    specs = _gb_specs(H, W)[:2] + [("src", (H, W, 4), dt), ("out", (H, W, 4), dt), ("fb", (H, W, 4), dt)]
    for planted in (False, True):
        rng = np.random.default_rng(11)
        src = _atrous_src(rng, f, storage) if planted else np.concatenate(
            [f["radiance"][..., :3] * 1.2 - 0.05, rng.uniform(-0.01, 0.05, (H, W, 1)).astype(np.float32)], -1).astype(dt)
        d = F.Denoiser(W, H, F.Params(storage=storage, variant=variant, phi_colour=PHI_C, phi_normal=PHI_N))
        gbs = G.gb_dev(f)
        mid, fb0, two = d.new_colour(), d.new_colour(), d.new_colour()
        d.FilterKernel(G.dev(src), mid, fb0, gbs, 1, 0)
        d.FilterKernel(mid, two, None, gbs, 2, 1)
        torch.cuda.synchronize()
        mid, two = G.host(mid), G.host(two)
        d.set_rows(rb, re)
        inputs = {"motion": f["motion"], "normal": f["normal"], "src": src}

        def call(ar):
            d.FilterKernelPair(ar.view("src"), ar.view("out"), ar.view("fb"), F.GBuffer(ar.view("motion"), ar.view("normal"), None))
        what = f"a-trous pair {W}x{H} {storage} {variant} rows {rb}..{re}{' with NaN and -0.0 texels' if planted else ''}"
        got, _ = in_arenas(specs, inputs, call, margin_rows=6 + 8, what=what, like={"out": "src", "fb": "src"})
        d.close()
        out, fb = got["out"], got["fb"]
        inrows = np.zeros((H, W), bool); inrows[rb:re] = True
        assert _written(out)[inrows].all() and PA.is_sentinel_array(out)[~inrows].all(), what + ": `out` is written on the launch rows and nowhere else"
        fbrows = np.zeros((H, W), bool); fbrows[max(0, rb - 4):min(H, re + 4)] = True
        assert PA.is_sentinel_array(fb)[~fbrows | sky].all(), what + ": feedback written outside the launch rows + 4, or on sky"
        o, t = out[rb:re], two[rb:re]
        if not planted:
            assert _same_bits(o, t), what + ": `out` differs from two svgf_atrous calls"
            assert _same_bits(fb[fbrows & ~sky], mid[fbrows & ~sky]), what + ": feedback differs from iteration 0"
            # against the oracle: its iteration 1 of the device's own iteration 0 (identical inputs: the stage tolerance holds)
            want = np.zeros_like(src)
            oracle.atrous(W, H, storage, mid, want, None, gbuf(f), step=2, phi_colour=PHI_C, phi_normal=PHI_N, iteration=1)
        else:
            g, w = o.astype(np.float32), t.astype(np.float32)
            assert np.array_equal(np.isnan(g), np.isnan(w)), what + ": NaN masks differ from two svgf_atrous calls"
            with np.errstate(all="ignore"):
                err = np.abs(np.nan_to_num(g, posinf=0, neginf=0) - np.nan_to_num(w, posinf=0, neginf=0)).max()
            assert err <= (2e-4 * max(1.0, 50.0 / PHI_C) if storage == "f32" else 2e-2), what + f": {err:.3e} from two svgf_atrous calls"
            assert np.array_equal(o[t == 0] == 0, t[t == 0] == 0) and np.array_equal(np.signbit(o[t == 0]), np.signbit(t[t == 0])), \
                what + ": sign of zero differs from two svgf_atrous calls"
            # against the oracle's two iterations: the feedback at the stage tolerance (the two device forms are each within it of the
            # oracle's iteration 0), `out` by its NaN mask and its zeros (tests/fuzz_parity.py:trial_pair holds no value of it to the oracle)
            want0, want = np.zeros_like(src), np.zeros_like(src)
            oracle.atrous(W, H, storage, src, want0, None, gbuf(f), step=1, phi_colour=PHI_C, phi_normal=PHI_N, iteration=0)
            oracle.atrous(W, H, storage, want0, want, None, gbuf(f), step=2, phi_colour=PHI_C, phi_normal=PHI_N, iteration=1)
            m = fbrows & ~sky
            if m.any():
                assert_close_with_nan(G, fb[m].reshape(-1, 4), want0[m].reshape(-1, 4), storage, what + ": feedback against the oracle's iteration 0")
            assert np.array_equal(np.isnan(g), np.isnan(want[rb:re].astype(np.float32))), what + ": NaN masks differ from the oracle's two iterations"
        want = want[rb:re]
        if not planted:
            assert_close_with_nan(G, o, want, storage, what + ": `out` against the oracle's iteration 1")
        assert _same_bits(o[sky[rb:re]], want[sky[rb:re]]), what + ": sky copy"
        zero = want == 0
        assert np.array_equal(o[zero] == 0, want[zero] == 0) and np.array_equal(np.signbit(o[zero]), np.signbit(want[zero])), what + ": sign of zero"


# ------------------------------------------------------------------ TAA, adapter, albedo
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("variant", ["auto", "direct"])
@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_taa(G, oracle, storage, variant, size):
    """taa_lds_kernel (its 68 x 12 staged texels start 3 up-left of the tile) and taa_kernel; test_gpu_parity.py:test_taa's comparison."""
    from svgf_amd import filter as F
    W, H = size
    dt = CDT[storage]
    rng = np.random.default_rng(31)
    filt = rng.uniform(-0.1, 1.2, (H, W, 4)).astype(dt)
    hist = rng.uniform(0, 1, (H, W, 4)).astype(dt)
    want = np.zeros_like(filt)
    oracle.taa(W, H, storage, filt, hist, want)
    specs = [("filtered", (H, W, 4), dt), ("history", (H, W, 4), dt), ("out", (H, W, 4), dt)]
    d = F.Denoiser(W, H, F.Params(storage=storage, variant=variant))
    what = f"TAA {W}x{H} {storage} {variant}"
    got, _ = in_arenas(specs, {"filtered": filt, "history": hist}, lambda ar: d.TAA(ar.view("filtered"), ar.view("history"), ar.view("out")),
                       margin_rows=3 + 8, what=what, like={"out": "filtered"})
    d.close()
    assert _written(got["out"]).all(), what
    if storage == "f32":
        assert np.abs(got["out"].astype(np.float64) - want.astype(np.float64)).max() <= 2e-6, what      # hardware exp2 / log2 in sRGB
    else:
        assert half_ulp_diff(got["out"], want).max() <= 1, what


@pytest.mark.parametrize("size", SIZES)
def test_pack_gbuffer(G, oracle, size):
    """svgf_pack_gbuffer: ddepth reads the 2x2 quad partner across the last row and the last column (odd W and H: the partner lies outside)."""
    from svgf_amd import filter as F
    from tests.test_gpu_parity import _look_at, _perspective
    W, H = size
    rng = np.random.default_rng(5)
    eye0, eye1 = np.array([0.3, 0.4, 5.0]), np.array([0.35, 0.38, 5.02])
    proj = _perspective(0.9, W / H, 0.1, 100.0)
    cm = lambda m: m.T.astype(np.float32).ravel()               # noqa: E731
    vp, pvp = cm(proj @ _look_at(eye1, (0, 0, 0))), cm(proj @ _look_at(eye0, (0, 0, 0)))
    pos = np.concatenate([rng.uniform(-2, 2, (H, W, 3)), rng.integers(0, 900, (H, W, 1))], -1).astype(np.float32)
    nrm = np.concatenate([rng.normal(size=(H, W, 3)), rng.integers(0, 20, (H, W, 1))], -1).astype(np.float32)
    nrm[rng.uniform(size=(H, W)) < 0.1, :3] = 0
    bary = np.concatenate([rng.uniform(0, 1, (H, W, 3)), rng.integers(0, 50, (H, W, 1))], -1).astype(np.float32)
    want = oracle.pack_gbuffer(pos, nrm, bary, vp, pvp, eye1.astype(np.float32))
    specs = [("position", (H, W, 4), np.float32), ("normal_in", (H, W, 4), np.float32), ("bary", (H, W, 4), np.float32)] + _gb_specs(H, W)
    d = F.Denoiser(W, H, F.Params(storage="f32"))
    cam = F.CameraC((C.c_float * 16)(*map(float, vp)), (C.c_float * 16)(*map(float, pvp)), (C.c_float * 3)(*map(float, eye1)))

    def call(ar):
        rc = d.lib.svgf_pack_gbuffer(d._h, *[F._ptr(ar.view(n)) for n in ("position", "normal_in", "bary")], C.byref(cam),
                                     *[F._ptr(ar.view(n)) for n in ("motion", "normal", "uv")])
        assert rc == 0
    what = f"pack_gbuffer {W}x{H}"
    got, _ = in_arenas(specs, {"position": pos, "normal_in": nrm, "bary": bary}, call, margin_rows=1 + 8, what=what,
                       like={"motion": "position"})
    d.close()
    for n, w in zip(("motion", "normal", "uv"), want):
        assert _written(got[n]).all(), f"{what}: {n} not written everywhere"
        assert np.array_equal(got[n].view(np.uint8), np.ascontiguousarray(w).view(np.uint8)), f"{what}: {n}"


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_albedo(G, oracle, storage, size):
    """svgf_demodulate into a third plane; svgf_modulate in place (out == in: the aliased plane is an output)."""
    from svgf_amd import filter as F
    W, H = size
    dt = CDT[storage]
    rng = np.random.default_rng(78)
    x = rng.uniform(0, 1, (H, W, 4)).astype(dt)
    alb = rng.uniform(-0.1, 1, (H, W, 4)).astype(dt)
    want_d = np.zeros_like(x); want_m = np.zeros_like(x)
    oracle.albedo(0, W, H, storage, x, alb, want_d)
    oracle.albedo(1, W, H, storage, want_d, alb, want_m)
    d = F.Denoiser(W, H, F.Params(storage=storage))
    what = f"albedo {W}x{H} {storage}"
    specs = [("x", (H, W, 4), dt), ("albedo", (H, W, 4), dt), ("out", (H, W, 4), dt)]
    got, _ = in_arenas(specs, {"x": x, "albedo": alb}, lambda ar: d.Demodulate(ar.view("x"), ar.view("albedo"), ar.view("out")),
                       margin_rows=8, what=what + " demodulate", like={"out": "x"})
    assert np.array_equal(got["out"].view(np.uint8), want_d.view(np.uint8)), what + ": demodulate"
    got, _ = in_arenas(specs[:2], {"albedo": alb}, lambda ar: d.Modulate(ar.view("x"), ar.view("albedo"), ar.view("x")),
                       margin_rows=8, what=what + " modulate in place", prefill={"x": want_d})
    assert np.array_equal(got["x"].view(np.uint8), want_m.view(np.uint8)), what + ": modulate"
    d.close()


# ------------------------------------------------------------------ strip contexts
@pytest.mark.parametrize("variant", ["auto", "direct"])
@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_strip_contexts(G, storage, variant):
    """A strip cut from the middle of the frame: the arena holds rows [y0, y0 + rows) only, so "inside the frame" and "inside the plane" differ on
    both sides — where row_ok, the zero-length resource and the strip guard of the reprojection earn their keep.  The owned rows equal the same
    rows of the whole-frame call bit for bit; rows outside svgf_set_rows stay the sentinel; the halo-violation count is the host's."""
    import torch
    from svgf_amd import filter as F
    from tests import camera_scene as cs
    W, H = FULL
    dt = CDT[storage]
    step = 4
    y0, rows, ob, oe = 60, 70, 60 + 2 * step, 130 - 2 * step          # the strip holds exactly the a-trous halo of its owned rows
    sl = slice(y0, y0 + rows)
    cut = lambda a: np.ascontiguousarray(a[sl])                         # noqa: E731
    f0, f1, prev, mom_prev, hist_prev, cur = _temporal_inputs(W, H, storage, "pan")
    f1["motion"][ob:oe:7, ::5, 1] = -40.0                              # some reprojections land in the frame but outside the strip
    f1["motion"][ob:oe:7, 1::5, 1] = 55.0
    P = F.Params(storage=storage, variant=variant, phi_colour=PHI_C, phi_normal=PHI_N)
    whole, d = F.Denoiser(W, H, P), F.Denoiser(W, H, P, strip=(y0, rows, ob, oe))
    gw = G.gb_dev(f1)
    # ---- a-trous and moments: against the whole-frame call
    src = _atrous_src(np.random.default_rng(5), f1, storage)
    src[ob, 5, 0] = np.nan; src[oe - 1, 9] = -0.0
    hist = np.random.default_rng(6).integers(1, 8, (H, W)).astype(np.uint8)
    wa, wf, wm = whole.new_colour(), whole.new_colour(), whole.new_colour()
    whole.FilterKernel(G.dev(src), wa, wf, gw, step, 0)
    whole.FilterMoments(G.dev(src), wm, G.dev(mom_prev), gw, G.dev(hist))
    torch.cuda.synchronize()
    wa, wf, wm = G.host(wa), G.host(wf), G.host(wm)
    specs = _gb_specs(rows, W)[:2] + [("src", (rows, W, 4), dt), ("out", (rows, W, 4), dt), ("fb", (rows, W, 4), dt), ("mom", (rows, W, 2), dt), ("hist", (rows, W), np.uint8)]
    inputs = {"motion": cut(f1["motion"]), "normal": cut(f1["normal"]), "src": cut(src), "mom": cut(mom_prev), "hist": cut(hist)}
    z = f1["motion"][..., 2]
    sky = ((z == 0) | (z == np.float32(1e30)))[sl]
    own = np.zeros((rows, W), bool); own[ob - y0:oe - y0] = True

    def atrous(ar):
        d.FilterKernel(ar.view("src"), ar.view("out"), ar.view("fb"), F.GBuffer(ar.view("motion"), ar.view("normal"), None), step, 0)
    what = f"strip a-trous {storage} {variant}"
    got, _ = in_arenas(specs, inputs, atrous, margin_rows=2 * step + 8, what=what, like={"out": "src", "fb": "src"})
    assert PA.is_sentinel_array(got["out"])[~own].all() and PA.is_sentinel_array(got["fb"])[~own | sky].all(), what + ": written outside the owned rows"
    assert _same_bits(got["out"][own], wa[sl][own]), what + ": owned rows differ from the whole frame"
    assert _same_bits(got["fb"][own & ~sky], wf[sl][own & ~sky]), what + ": feedback differs from the whole frame"

    def moments(ar):
        d.FilterMoments(ar.view("src"), ar.view("out"), ar.view("mom"), F.GBuffer(ar.view("motion"), ar.view("normal"), None), ar.view("hist"))
    what = f"strip moments {storage} {variant}"
    got, _ = in_arenas(specs, inputs, moments, margin_rows=3 + 8, what=what, like={"out": "src", "fb": "src"})
    assert PA.is_sentinel_array(got["out"])[~own].all() and PA.is_sentinel_array(got["fb"]).all(), what + ": written outside the owned rows"
    assert _same_bits(got["out"][own], wm[sl][own]), what + ": owned rows differ from the whole frame"
    # ---- a narrower row range: rows outside svgf_set_rows stay as they were
    d.set_rows(ob + 5, oe - 9)
    what = f"strip a-trous {storage} {variant} rows {ob + 5}..{oe - 9}"
    got, _ = in_arenas(specs, inputs, atrous, margin_rows=2 * step + 8, what=what, like={"out": "src", "fb": "src"})
    sub = np.zeros((rows, W), bool); sub[ob + 5 - y0:oe - 9 - y0] = True
    assert PA.is_sentinel_array(got["out"])[~sub].all() and _same_bits(got["out"][sub], wa[sl][sub]), what
    d.set_rows(-1, -1)
    # ---- temporal: the valid rows narrower than the strip, reprojections beyond them counted
    v0, v1 = y0 + 3, y0 + rows - 2
    d.set_valid_rows(v0, v1)
    _, qy, inside = cs.reprojection(f1)
    want_violations = int((inside[ob:oe] & ~((qy[ob:oe] >= v0) & (qy[ob:oe] < v1))).sum())
    assert want_violations > 50
    wc, wh, wmo = whole.new_colour(), whole.new_history(), whole.new_moments()
    whole.TemporalFilter(G.dev(prev), G.dev(cur), wc, gw, G.gb_dev(f0), G.dev(hist_prev), wh, wmo, G.dev(mom_prev))
    torch.cuda.synchronize()
    wc, wh, wmo = G.host(wc), G.host(wh), G.host(wmo)
    kept = own & ~(inside & ~((qy >= v0) & (qy < v1)))[sl]            # (a violating pixel is a rejection: no longer the whole frame's)
    specs = _gb_specs(rows, W, "c_") + _gb_specs(rows, W, "p_") + [("prev", (rows, W, 4), dt), ("radiance", (rows, W, 4), dt), ("colour", (rows, W, 4), dt),
             ("mom_prev", (rows, W, 2), dt), ("mom", (rows, W, 2), dt), ("hist_prev", (rows, W), np.uint8), ("hist", (rows, W), np.uint8)]
    inputs = {**{k: cut(v) for k, v in _gb_in(f1, "c_").items()}, **{k: cut(v) for k, v in _gb_in(f0, "p_").items()}, "prev": cut(prev), "radiance": cut(cur),
              "mom_prev": cut(mom_prev), "hist_prev": cut(hist_prev)}

    def temporal(ar):
        d.TemporalFilter(ar.view("prev"), ar.view("radiance"), ar.view("colour"), _gb_of(F, ar, "c_"), _gb_of(F, ar, "p_"),
                         ar.view("hist_prev"), ar.view("hist"), ar.view("mom"), ar.view("mom_prev"))
        return d.halo_violations(clear=True)
    what = f"strip temporal {storage} {variant}"
    got, violations = in_arenas(specs, inputs, temporal, margin_rows=55 + 8, what=what, like={"colour": "prev", "mom": "mom_prev", "hist": "hist_prev"})
    assert violations == want_violations, f"{what}: {violations} halo violations, the host counts {want_violations}"
    assert PA.is_sentinel_array(got["colour"])[~own].all() and PA.is_sentinel_array(got["mom"])[~own].all() and (got["hist"][~own] == PA.BYTE_SENTINEL).all(), what
    assert _same_bits(got["colour"][kept], wc[sl][kept]) and _same_bits(got["mom"][kept], wmo[sl][kept]) and np.array_equal(got["hist"][kept], wh[sl][kept]), what
    assert (got["hist"][own & ~kept] == 1).all(), what + ": a reprojection beyond the valid rows is a rejection"
    d.close(); whole.close()


# ------------------------------------------------------------------ the frame driver
@pytest.mark.parametrize("prev_guide", [False, True])
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_denoise_frame(G, storage, size, prev_guide):
    """svgf_denoise_frame with radiance, cur and prev in an arena (the state planes are the context's own): three cold frames and three steady
    ones.  The result and the four state planes hold the same bits under every fill, and those of a run on stand-alone planes."""
    import torch
    from svgf_amd import filter as F
    W, H = size
    dt = CDT[storage]
    N = 6
    fr = [synth.make_frame(W, H, k, mv=(-2.5, 1.5)) for k in range(N)]
    P = F.Params(storage=storage, steps=3)
    PLANES = (F.PLANE_COLOUR, F.PLANE_MOMENTS, F.PLANE_FILTER, F.PLANE_HISTORY)

    def state(d):
        torch.cuda.synchronize()
        return [G.host(t).copy() for p in PLANES for i in (0, 1) if (t := d.state_plane(p, i)) is not None]
    # stand-alone planes (two G-buffers that alternate, as the reference's Framebuffer[PingPongInx])
    d = F.Denoiser(W, H, P)
    d.set_prev_guide(prev_guide)
    gbs = [G.gb_dev(fr[0]), G.gb_dev(fr[1])]
    alone = []
    for k in range(N):
        if k >= 2:
            for t, n in zip((gbs[k & 1].motion, gbs[k & 1].normal, gbs[k & 1].uv), ("motion", "normal", "uv")):
                t.view(torch.uint8).copy_(G.dev(fr[k][n]).view(torch.uint8))
        res = G.host(d.Render(G.dev(fr[k]["radiance"].astype(dt)), gbs[k & 1], gbs[1 - (k & 1)] if k else None)).copy()
        alone.append([res] + state(d))
    d.close()
    specs = _gb_specs(H, W, "a_") + _gb_specs(H, W, "b_") + [("radiance", (H, W, 4), dt)]
    for li, (fill, tight) in enumerate(LAYOUTS):
        offs = {name: PA.OFFSETS[(i + li) % 3] for i, (name, _, _) in enumerate(specs)}
        ar = PA.Arena(specs, {**_gb_in(fr[0], "a_"), **_gb_in(fr[1], "b_"), "radiance": fr[0]["radiance"].astype(dt)}, fill=fill, tight=tight,
                      margin_rows=2 * 4 + 8, offsets=offs, seed=li)
        d = F.Denoiser(W, H, P)
        d.set_prev_guide(prev_guide)
        gb = [_gb_of(F, ar, "a_"), _gb_of(F, ar, "b_")]
        for k in range(N):
            what = f"frame driver {W}x{H} {storage} prev_guide {prev_guide} [{fill}{', tight' if tight else ''}] frame {k}"
            if k >= 2:
                for n in ("motion", "normal", "uv"):
                    ar.view("ab"[k & 1] + "_" + n).view(torch.uint8).copy_(G.dev(fr[k][n]).view(torch.uint8))
            ar.view("radiance").copy_(G.dev(fr[k]["radiance"].astype(dt)))
            torch.cuda.synchronize()
            ar.snapshot_inputs(*[n for n, _, _ in specs])
            res = G.host(d.Render(ar.view("radiance"), gb[k & 1], gb[1 - (k & 1)] if k else None)).copy()
            got = [res] + state(d)
            ar.check(what)
            assert len(got) == len(alone[k]) == 1 + 2 * len(PLANES), what
            for i, (g, w) in enumerate(zip(got, alone[k])):
                assert _same_bits(g, w), what + f": {'the result' if i == 0 else f'state plane {PLANES[(i - 1) // 2]}[{(i - 1) % 2}]'} differs from the run on stand-alone planes"
        d.close()
