"""The rows of a launch and a frame's choice of moments kernel are ARGUMENTS of the stage helpers behind the C ABI (svgf_amd/csrc/svgf_ctx.h),
not state of the context: what svgf_set_rows set stays what it was whatever a driver launched or a call refused in between, and what a driver
decided for its frame (the streaming moments kernel of a cold or crowded frame: a temporal launch that appends to no list) never reaches a stage
call on the same context.  Every comparison is on raw bits, fp32 storage."""
import ctypes as C

import numpy as np
import pytest

from tests.helpers import frames

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_HALO = -1, -4
SENTINEL = 0x7FA5A5A5            # a NaN payload no launch produces from finite inputs


@pytest.fixture(scope="module")
def G():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tests import gpu_helpers
    return gpu_helpers


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _sentinel_plane(rows, W):
    import torch
    return torch.full((rows, W, 4), SENTINEL, dtype=torch.int32, device="cuda:0")


def _bits(G, t):
    return G.host(t).view(np.uint32)


def _strip_planes(G, fr, y0, y1):
    """The rows [y0, y1) of a synthetic frame as device planes: (radiance as a colour plane, G-buffer)."""
    from svgf_amd import filter as F
    sl = slice(y0, y1)
    gb = F.GBuffer(*(G.dev(np.ascontiguousarray(fr[k][sl])) for k in ("motion", "normal", "uv")))
    return G.dev(np.ascontiguousarray(fr["radiance"][sl].astype(np.float32))), gb


def test_refused_calls_leave_the_rows_of_the_context_alone(G):
    """A strip context with svgf_set_rows(20, 36) refuses three calls — moments rows outside the temporal rows, a step whose reach the strip does
    not hold, an in-place pair launch — and the next svgf_atrous still computes exactly rows [20, 36)."""
    import torch
    from svgf_amd import filter as F
    W, H, strip, rows = 96, 64, (8, 48, 16, 40), (20, 36)
    fr = frames(W, H, 1, mv=(1.0, -0.5))[0]
    src, gb = _strip_planes(G, fr, strip[0], strip[0] + strip[1])

    def make():
        d = F.Denoiser(W, H, F.Params(storage="f32", steps=3), strip=strip)
        d.set_rows(*rows)
        return d

    def step1(d):
        out = _sentinel_plane(strip[1], W)
        d.FilterKernel(src, out, None, gb, 1, 1)
        torch.cuda.synchronize()
        return _bits(G, out)

    fresh = make()
    want = step1(fresh)
    fresh.close()

    d = make()
    lib, h = d.lib, d._h
    col, col2, filt, mom, mom2, hist, hist2 = d.new_colour(), d.new_colour(), d.new_colour(), d.new_moments(), d.new_moments(), d.new_history(), d.new_history()
    rc = lib.svgf_temporal_moments(h, _p(col), _p(src), _p(col2), _p(filt), gb.c, gb.c, _p(hist), _p(hist2), _p(mom), _p(mom2), 12, 36, 0)
    assert rc == ERR_INVALID, (rc, lib.svgf_last_error(h))
    assert lib.svgf_atrous(h, _p(src), _p(filt), None, gb.c, 8, 3) == ERR_HALO          # reach 16: rows [4, 52) of a strip that holds [8, 56)
    assert lib.svgf_atrous_pair(h, _p(src), _p(src), _p(col), gb.c) == ERR_INVALID
    got = step1(d)
    d.close()

    lo, hi = rows[0] - strip[0], rows[1] - strip[0]
    assert not (want[lo:hi] == SENTINEL).any(), "the fresh context did not write its rows"
    assert np.array_equal(got[lo:hi], want[lo:hi])
    assert (got[:lo] == SENTINEL).all() and (got[hi:] == SENTINEL).all(), "rows outside svgf_set_rows were written"


def test_a_strip_drivers_context_keeps_its_owned_rows(G):
    """After two frames of the strip driver a stage call on svgf_strips_context computes the strip's OWNED rows, as svgf_create_strip's default
    does — not the rows of whichever launch the driver enqueued last — and the driver's next frame is still the whole frame's, bit for bit."""
    import torch
    from svgf_amd import filter as F
    from svgf_amd import strips
    W, H, world, steps = 128, 96, 2, 2
    P = F.Params(storage="f32", steps=steps)
    fr = frames(W, H, 3, mv=(1.0, -1.5))
    whole = G.HipPipeline(W, H, "f32", steps=steps)
    gbs = [G.gb_dev(f) for f in fr]
    want = [whole.frame(fr[k]["radiance"], gbs[k], gbs[max(k - 1, 0)]) for k in range(3)]
    drv = strips.NativeStrips(W, H, world, P, list(range(world)), [0] * world, plan="per-iteration", motion_reach=2, transport="mailbox")
    inputs = [[_strip_planes(G, f, lay["y0"], lay["y1"]) for lay in drv.layouts] for f in fr]
    torch.cuda.synchronize()

    def drive(k):
        outs = drv.frame([c[0] for c in inputs[k]], [c[1] for c in inputs[k]], [c[1] for c in inputs[k - 1]] if k else None)
        drv.sync()
        got = np.concatenate([G.host(drv.owned(r, o)) for r, o in enumerate(outs)], 0)
        assert np.array_equal(got.view(np.uint8), want[k].view(np.uint8)), f"frame {k}"

    drive(0)
    drive(1)
    for r in range(world):
        ctx = drv.lib.svgf_strips_context(drv._h, r)
        st = F.StripC()
        assert drv.lib.svgf_get_size(ctx, None, None, C.byref(st)) == 0
        assert (st.y0, st.y0 + st.rows, (st.own_begin, st.own_end)) == (drv.layouts[r]["y0"], drv.layouts[r]["y1"], drv.layouts[r]["own"])
        src, gb = inputs[2][r]
        out = _sentinel_plane(st.rows, W)
        assert drv.lib.svgf_atrous(ctx, _p(src), _p(out), None, gb.c, 1, 1) == 0, drv.lib.svgf_last_error(ctx)
        ref = F.Denoiser(W, H, P, strip=(st.y0, st.rows, st.own_begin, st.own_end))
        ref_out = _sentinel_plane(st.rows, W)
        ref.FilterKernel(src, ref_out, None, gb, 1, 1)
        torch.cuda.synchronize()
        ref.close()
        got, exp = _bits(G, out), _bits(G, ref_out)
        lo, hi = st.own_begin - st.y0, st.own_end - st.y0
        assert not (exp[lo:hi] == SENTINEL).any(), "the strip context did not write its owned rows"
        assert np.array_equal(got[lo:hi], exp[lo:hi]), f"rank {r}"
        assert (got[:lo] == SENTINEL).all() and (got[hi:] == SENTINEL).all(), f"rank {r}: rows outside the owned ones were written"
    drive(2)
    drv.close()


@pytest.fixture(scope="module")
def partly_young(G):
    """Inputs of one svgf_temporal_moments call at 192x32 (three 64-column segments per row) whose previous history is >= 4 in the left
    segment, 0 in the right one and alternates 0 / 8 per pixel in the middle one — one wave in three is partly young and goes through the
    list — and what a context that has run nothing makes of them."""
    W, H = 192, 32
    fr = frames(W, H, 5, mv=(0.0, 0.0))
    hist_prev = np.zeros((H, W), np.uint8)
    hist_prev[:, :64] = 8
    hist_prev[:, 64:128:2] = 0
    hist_prev[:, 65:128:2] = 8
    rng = np.random.default_rng(7)
    inp = dict(W=W, H=H, fr=fr, gbs=[G.gb_dev(f) for f in fr], hist_prev=G.dev(hist_prev), radiance=G.dev(fr[4]["radiance"].astype(np.float32)),
               prev_colour=G.dev(fr[3]["radiance"].astype(np.float32)), mom_prev=G.dev(rng.random((H, W, 2), dtype=np.float32)))
    inp["want"] = _temporal_moments(G, inp, warm_frames=0)
    hist = inp["want"]["hist"][8:]           # (below the scene's sky, whose texels never reproject: history 1 whatever it was)
    assert (hist[:, 64:128] < 4).any(axis=1).all() and (hist[:, 64:128] >= 4).any(axis=1).all(), "the middle segment is not partly young"
    assert (hist[:, :64] >= 4).all() and (hist[:, 128:] < 4).all()
    return inp


def _temporal_moments(G, inp, warm_frames):
    """`warm_frames` frames of svgf_denoise_frame, then the stage call on caller planes -> the raw bits of everything it wrote."""
    import torch
    from svgf_amd import filter as F
    d = F.Denoiser(inp["W"], inp["H"], F.Params(storage="f32", steps=3))
    for k in range(warm_frames):
        d.Render(G.dev(inp["fr"][k]["radiance"].astype(np.float32)), inp["gbs"][k], inp["gbs"][max(k - 1, 0)])
    colour_out, filter_out, mom_cur, hist_cur = d.new_colour(), d.new_colour(), d.new_moments(), d.new_history()
    d.TemporalMoments(inp["prev_colour"], inp["radiance"], colour_out, filter_out, inp["gbs"][4], inp["gbs"][4], inp["hist_prev"], hist_cur, mom_cur,
                      inp["mom_prev"], feedback_follows=False)
    torch.cuda.synchronize()
    got = dict(colour=_bits(G, colour_out), filter=_bits(G, filter_out), mom=_bits(G, mom_cur), hist=G.host(hist_cur))
    d.close()
    return got


@pytest.mark.parametrize("warm_frames", [1, 4])
def test_the_drivers_moments_choice_does_not_reach_the_stage_calls(G, partly_young, warm_frames):
    """svgf_denoise_frame served its frame(s) — one: a cold frame, the streaming kernel, a temporal launch that appends to no list; four: past
    the cold start — and svgf_temporal_moments on the same context still appends its partly young waves: the same bits as on a fresh context."""
    got = _temporal_moments(G, partly_young, warm_frames)
    for name, want in partly_young["want"].items():
        assert np.array_equal(got[name], want), name
