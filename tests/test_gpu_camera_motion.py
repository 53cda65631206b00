"""The filter on per-pixel motion from a moving camera (tests/camera_scene.py): orbit, dolly, roll, a fast diagonal pan and a whip turn,
each with an object that moves by itself.  Every other sequence of the suite reprojects with one motion vector for the whole frame, so the
64 lanes of a wave always gathered from one shifted row segment and young pixels sat in border bands only.

  a  temporal against the oracle, raw bits, every path, both storages, mesh-ID test on and off, at a ragged size;
  b  moments and a-trous (steps 1-16) under direct / lds / lds-general from the oracle's own inputs, at the stage tolerances;
  c  eight frames free-running against the oracle: identical masks, colour within FREE_RUNNING;
  d  the frame driver against the stage calls, bit for bit, under its settings, and svgf_adaptive_moments_sample against a host restatement;
  e  the strip driver (mailbox transport) against the frame driver, and the halo-violation count against a host count when the reach is short;
  f  one orbit at 3840x2160: temporal bit-exact, stages within tolerance, frame driver == stage calls;
  g  TAA and the G-buffer adapter on strip contexts and row ranges;
  h  the C++ drop-in (include/SVGF.h) over a real sequence with distinct current and previous G-buffers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import camera_scene as cs
from tests import launch_geometry as LG
from tests.helpers import CDT, free_running_bounds, free_running_envelope, gbuf
from tests.plane_arena import BYTE_SENTINEL

pytestmark = pytest.mark.gpu

W, H = 517, 333
NT = min(16, int(os.environ.get("OMP_NUM_THREADS") or 8))
MOVING = (1.0, 0.0)                         # (free_running_bounds: the bounds of a moving camera)


@pytest.fixture(scope="module")
def G():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tests import gpu_helpers
    return gpu_helpers


def _seq(path, N, w=W, h=H):
    return cs.sequence(path, w, h, N)


def _adapter_matches(G, fr):
    """The device adapter against the oracle's (which made the planes), bit for bit: the chain from adapter to filter."""
    from svgf_amd import filter as F
    h, w = fr["motion"].shape[:2]
    d = F.Denoiser(w, h, F.Params())
    gb = d.PackGBuffer(G.dev(fr["position"]), G.dev(fr["normal_in"]), G.dev(fr["bary"]), fr["vp"], fr["prev_vp"], fr["eye"])
    assert np.array_equal(G.host(gb.motion).view(np.uint32), fr["motion"].view(np.uint32)), "adapter motion"
    assert np.array_equal(G.host(gb.normal).view(np.uint16), fr["normal"]) and np.array_equal(G.host(gb.uv).view(np.uint16), fr["uv"]), "adapter normal / uv"
    d.close()
    return gb


# ------------------------------------------------------------------ a
@pytest.mark.parametrize("storage", ["f32", "f16"])
@pytest.mark.parametrize("path", cs.PATHS)
def test_temporal_bit_exact_on_camera_paths(G, oracle, path, storage):
    from svgf_amd import filter as F
    fr = _seq(path, 8)
    _adapter_matches(G, fr[5])
    dt = CDT[storage]
    for mesh in (0, 1):
        ref = oracle.Pipeline(W, H, storage, steps=0, mesh_id_test=mesh, nthreads=NT)
        d = F.Denoiser(W, H, F.Params(storage=storage, mesh_id_test=mesh))
        gbs = [G.gb_dev(f) for f in fr]
        for k in range(len(fr)):
            kp = max(k - 1, 0)
            ref.frame(fr[k]["radiance"], gbuf(fr[k]), gbuf(fr[kp]))
            t = ref.taps
            col, hist, mom = d.new_colour(), d.new_history(), d.new_moments()
            d.TemporalFilter(G.dev(t["prev_colour"]), G.dev(t["radiance"]), col, gbs[k], gbs[kp], G.dev(t["prev_hist"]), hist, mom, G.dev(t["prev_mom"]))
            what = f"{path} {storage} mesh {mesh} frame {k}"
            assert np.array_equal(G.host(hist), t["hist"]), what + ": history"
            assert np.array_equal(G.host(col).view(np.uint8), t["temporal"].view(np.uint8)), what + ": colour"
            assert np.array_equal(G.host(mom).view(np.uint8), t["mom"].view(np.uint8)), what + ": moments"
        assert t["temporal"].dtype == dt and 0 < (t["hist"] > 1).mean() < 1
        d.close()


# ------------------------------------------------------------------ b
@pytest.mark.parametrize("storage", ["f32", "f16"])
@pytest.mark.parametrize("variant", ["direct", "lds", "lds-general"])
def test_stages_from_identical_inputs_on_camera_paths(G, oracle, variant, storage):
    """test_gpu_parity.py:test_pipeline_stagewise_identical_inputs on these G-buffers (its moments bounds, TOL for the a-trous iterations)."""
    from svgf_amd import filter as F
    for path in cs.PATHS:
        fr = _seq(path, 6)
        ref = oracle.Pipeline(W, H, storage, steps=5, nthreads=NT)
        d = F.Denoiser(W, H, F.Params(storage=storage, steps=5, variant=variant))
        gbs = [G.gb_dev(f) for f in fr]
        for k in range(len(fr)):
            kp = max(k - 1, 0)
            ref.frame(fr[k]["radiance"], gbuf(fr[k]), gbuf(fr[kp]))
            t = ref.taps
            what = f"{path} {variant} {storage} frame {k}"
            out = d.new_colour()
            d.FilterMoments(G.dev(t["temporal"]), out, G.dev(t["mom"]), gbs[k], G.dev(t["hist"]))
            got = G.host(out)
            keep = t["hist"] >= 4
            assert np.array_equal(got[keep].view(np.uint8), t["temporal"][keep].view(np.uint8)), what + ": steady pixels are copied"
            lim = 8e-5 if storage == "f32" else 1e-3
            assert np.abs(got.astype(np.float64) - t["moments"].astype(np.float64)).max() <= lim, what + ": moments"
            for i in range(5):
                fb = G.dev(t["temporal"]) if i == 0 else None
                d.FilterKernel(G.dev(t["atrous_in"][i]), out, fb, gbs[k], 1 << i, i)
                G.assert_colour_close(G.host(out), t["atrous_out"][i], storage, f"{what} a-trous step {1 << i}")
        d.close()


# ------------------------------------------------------------------ c
@pytest.mark.parametrize("storage", ["f32", "f16"])
@pytest.mark.parametrize("path", ["orbit", "dolly", "pan"])
def test_free_running_on_camera_paths(G, oracle, path, storage):
    """Eight frames, the device feeding itself.  Masks identical on every frame; the share of values beyond FREE_RUNNING's tight bound within its
    `frac`; the largest difference inside the ENVELOPE of the same frames (two correct CPU builds of the reference, tests/helpers.py).
    FREE_RUNNING's `loose` maximum was measured on the constant pan and does not carry over to this content: at frame 3, where the first pixels
    leave the spatial variance estimate with a temporal variance of exactly 0 (phi_l = PhiColour x 1e-5, Filter.cuh:562), the oracle and its
    all-fp32 FMA build already end up 0.2 apart in fp32 on these frames.  fp16 is held, like the pan, against the envelope build that models
    the GPU's 1-ulp transcendentals (helpers.py:FREE_RUNNING, inside_envelope)."""
    fr = list(_seq(path, 8))
    ref = oracle.Pipeline(W, H, storage, steps=5, nthreads=NT)
    hip = G.HipPipeline(W, H, storage, steps=5)
    gbs = [G.gb_dev(f) for f in fr]
    b = free_running_bounds(storage, MOVING)
    worst = 0.0
    for k in range(len(fr)):
        kp = max(k - 1, 0)
        want = ref.frame(fr[k]["radiance"], gbuf(fr[k]), gbuf(fr[kp])).astype(np.float64)
        got = hip.frame(fr[k]["radiance"], gbs[k], gbs[kp]).astype(np.float64)
        assert np.array_equal(hip.taps["hist"], ref.taps["hist"]), f"{path} frame {k}: history mask"
        err = np.abs(got - want)[..., :3]
        worst = max(worst, float(err.max()))
        assert (err > b["tight"] + 1e-5 * np.abs(want[..., :3])).mean() <= b["frac"], f"{path} {storage} frame {k}: share beyond the tight bound"
    env = free_running_envelope(oracle, fr, storage, flavour=b["inside_envelope"])      # (fp16: the 1-ulp transcendental model, as under the pan)
    assert env["mask_mismatches"] == 0
    assert worst <= env["max_abs"], f"{path} {storage}: device-vs-oracle {worst:.3e} outside the oracle-vs-oracle envelope {env['max_abs']:.3e}"


# ------------------------------------------------------------------ d
SETTINGS = ["default", "prev_guide", "in_flight", "pair", "adaptive_off"]


def _expected_sample(hist, normal):
    return cs.young_sample(cs.listed_young(hist, normal))


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("path", cs.PATHS)
def test_frame_driver_equals_stage_calls_on_camera_paths(G, path, setting):
    import torch
    from svgf_amd import filter as F
    N = 12
    storage = "f16" if (cs.PATHS.index(path) + SETTINGS.index(setting)) % 2 else "f32"
    fr = _seq(path, N)
    gbs = [G.gb_dev(f) for f in fr]
    hip = G.HipPipeline(W, H, storage, steps=5)
    d = F.Denoiser(W, H, F.Params(storage=storage, steps=5))
    if setting == "prev_guide":
        d.set_prev_guide(True)
    elif setting == "in_flight":
        d.set_frames_in_flight(2)
    elif setting == "pair":
        d.set_iteration_fusion(True)
    elif setting == "adaptive_off":
        d.set_adaptive_moments(False)
    states, hists = [], []
    for k in range(N):
        want = hip.frame(fr[k]["radiance"], gbs[k], gbs[max(k - 1, 0)])
        got = d.Render(G.dev(fr[k]["radiance"].astype(G.NPDT[storage])), gbs[k], gbs[k - 1] if k else None)
        d.sync()
        torch.cuda.synchronize()
        what = f"{path} {setting} {storage} frame {k}"
        assert np.array_equal(G.host(got).view(np.uint8), want.view(np.uint8)), what
        assert np.array_equal(G.host(d.state_plane(F.PLANE_HISTORY, 1 - d.pingpong())), hip.taps["hist"]), what + ": history"
        assert np.array_equal(G.host(d.state_plane(F.PLANE_MOMENTS, 1 - d.pingpong())).view(np.uint8), hip.taps["mom"].view(np.uint8)), what + ": moments"
        hists.append(hip.taps["hist"])
        states.append(d.adaptive_moments_state())
        # frame k's temporal launch published the sample of frame k - 1 (none from the three cold frames after a reset)
        want_s = _expected_sample(hists[k - 1], fr[k - 1]["normal"]) if k >= 4 else (0, 0)
        assert d.adaptive_moments_sample() == want_s, f"{what}: sample {d.adaptive_moments_sample()} != {want_s}"
    if setting == "adaptive_off":
        assert not any(states)
    if path == "whip" and setting != "adaptive_off":
        assert any(states) and not states[-1], f"the whip must switch the dense moments kernel on and off again: {states}"
    d.close()


# ------------------------------------------------------------------ e
def _strip_inputs(G, fr, lay, storage):
    from svgf_amd import filter as F
    sl = slice(lay["y0"], lay["y1"])
    gb = F.GBuffer(*(G.dev(np.ascontiguousarray(fr[k][sl])) for k in ("motion", "normal", "uv")))
    return G.dev(np.ascontiguousarray(fr["radiance"][sl].astype(G.NPDT[storage]))), gb


def _max_reach(fr):
    return max(int(np.abs(cs.rzi(f["motion"][..., 1])).max()) for f in fr)


def _host_violations(f, lay, H_):
    """Pixels of the temporal rows whose reprojection lands inside the frame but outside the rows holding valid state."""
    own0, own1 = lay["own"]
    rb, re = max(0, own0 - lay["ext_temporal"]), min(H_, own1 + lay["ext_temporal"])
    v0, v1 = max(lay["y0"], own0 - lay["halo_state"]), min(lay["y1"], own1 + lay["halo_state"])
    _, qy, inside = cs.reprojection(f)
    return int((inside[rb:re] & ~((qy[rb:re] >= v0) & (qy[rb:re] < v1))).sum())


STRIP_SIZE = (320, 960)
STRIP_PATHS = ("orbit", "dolly", "roll", "pan")


@pytest.mark.parametrize("plan", ["ghost", "grouped", "per-iteration"])
@pytest.mark.parametrize("world", [2, 3, 8])
def test_strips_equal_the_frame_driver_on_camera_paths(G, world, plan):
    import torch
    from svgf_amd import filter as F
    from svgf_amd import strips
    Ws, Hs = STRIP_SIZE
    i = [2, 3, 8].index(world) * 3 + ["ghost", "grouped", "per-iteration"].index(plan)
    path, storage, N = STRIP_PATHS[i % 4], ("f32", "f16")[i % 2], 4
    fr = _seq(path, N, Ws, Hs)
    reach = _max_reach(fr)
    assert reach >= 2, f"{path}: rows move by {reach} at most"
    P = F.Params(storage=storage, steps=5)
    whole = F.Denoiser(Ws, Hs, P)
    drv = strips.NativeStrips(Ws, Hs, world, P, list(range(world)), [0] * world, plan=plan, motion_reach=reach, transport="mailbox")
    gbs = [G.gb_dev(f) for f in fr]
    prev_in = None
    for k in range(N):
        want = G.host(whole.Render(G.dev(fr[k]["radiance"].astype(G.NPDT[storage])), gbs[k], gbs[k - 1] if k else None)).copy()
        cur_in = [_strip_inputs(G, fr[k], lay, storage) for lay in drv.layouts]
        torch.cuda.synchronize()
        outs = drv.frame([c[0] for c in cur_in], [c[1] for c in cur_in], [p[1] for p in prev_in] if prev_in else None)
        drv.sync()
        got = np.concatenate([G.host(drv.owned(r, o)) for r, o in enumerate(outs)], 0)
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), f"{path} world {world} {plan} {storage} reach {reach}: frame {k}"
        prev_in = cur_in
    drv.close()
    whole.close()


def _ctx_violations(drv, k):
    n = C.c_ulonglong()
    rc = drv.lib.svgf_halo_violations(drv.lib.svgf_strips_context(drv._h, k), C.byref(n), 0)
    assert rc == 0
    return n.value


def test_halo_violations_are_counted_pixel_for_pixel(G):
    """A reach below the largest |rzi(mv.y)|: every frame, each rank's count (read before the sync that reports and clears it) equals the
    host's count of the pixels of its temporal rows that reproject inside the frame but outside its valid rows — one reach where only a
    few pixels cross, one where many do; the same count through the stage calls of a strip context."""
    import torch
    from svgf_amd import filter as F
    from svgf_amd import strips
    Ws, Hs = STRIP_SIZE
    world, N, storage = 3, 4, "f32"
    fr = _seq("pan", N, Ws, Hs)
    full = _max_reach(fr)
    P = F.Params(storage=storage, steps=5)
    few_seen = many_seen = False
    for reach in (full // 2, 0):
        drv = strips.NativeStrips(Ws, Hs, world, P, list(range(world)), [0] * world, plan="grouped", motion_reach=reach, transport="mailbox")
        prev_in = None
        for k in range(N):
            cur_in = [_strip_inputs(G, fr[k], lay, storage) for lay in drv.layouts]
            torch.cuda.synchronize()
            drv.frame([c[0] for c in cur_in], [c[1] for c in cur_in], [p[1] for p in prev_in] if prev_in else None)
            want = [_host_violations(fr[k], lay, Hs) for lay in drv.layouts]
            got = [_ctx_violations(drv, r) for r in range(world)]
            assert got == want, f"reach {reach} frame {k}: device {got}, host {want}"
            if sum(want):
                few_seen |= sum(want) < 200
                many_seen |= sum(want) >= 200
                with pytest.raises(F.SvgfError, match="halo"):
                    drv.sync()
            else:
                drv.sync()
            prev_in = cur_in
        drv.close()
    assert few_seen and many_seen, "a frame where only a few pixels cross and one where many do"
    # the stage calls of a strip context: the temporal rows and valid rows of rank 1 set by hand
    lay = strips.strips_plan(Ws, Hs, 1, world, 5, "grouped", 3, 0)
    d = F.Denoiser(Ws, Hs, P, strip=(lay["y0"], lay["y1"] - lay["y0"], lay["own"][0], lay["own"][1]))
    own0, own1 = lay["own"]
    d.set_rows(max(0, own0 - lay["ext_temporal"]), min(Hs, own1 + lay["ext_temporal"]))
    d.set_valid_rows(max(lay["y0"], own0 - lay["halo_state"]), min(lay["y1"], own1 + lay["halo_state"]))
    rad, gb1 = _strip_inputs(G, fr[2], lay, storage)
    _, gb0 = _strip_inputs(G, fr[1], lay, storage)
    d.TemporalFilter(d.new_colour(), rad, d.new_colour(), gb1, gb0, d.new_history(), d.new_history(), d.new_moments(), d.new_moments())
    want = _host_violations(fr[2], lay, Hs)
    assert want > 0 and d.halo_violations(clear=True) == want
    d.close()


# ------------------------------------------------------------------ f
@pytest.fixture(scope="module")
def cus(G):
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def test_orbit_at_4k(G, oracle, cus):
    """Temporal bit-exact, moments and a-trous within tolerance against the oracle, and the frame driver equal to the stage calls, over four
    frames of the orbit at 3840x2160 (the long streaming bands, asserted as test_gpu_fullsize_parity.py does)."""
    import torch
    from svgf_amd import filter as F
    W4, H4, N, storage = 3840, 2160, 4, "f32"
    mg = LG.moments_lds(W4, H4, cus)
    assert mg["band"] > LG.constants()["kAtrousMinBand"], mg
    for S in (1, 2, 4, 8, 16):
        geo = LG.atrous_lds(W4, H4, S, cus)
        assert geo["band"] > LG.constants()["kAtrousMinBand"] and geo["xgroup"] > 1, (S, geo)
    fr = [cs.make_frame("orbit", k, W4, H4) for k in range(N)]
    _adapter_matches(G, fr[1])
    gbs = [G.gb_dev(f) for f in fr]
    ref = oracle.Pipeline(W4, H4, storage, steps=5, nthreads=NT)
    d = F.Denoiser(W4, H4, F.Params(storage=storage, steps=5))
    hip = G.HipPipeline(W4, H4, storage, steps=5)
    drv = F.Denoiser(W4, H4, F.Params(storage=storage, steps=5))
    for k in range(N):
        kp = max(k - 1, 0)
        ref.frame(fr[k]["radiance"], gbuf(fr[k]), gbuf(fr[kp]))
        t = ref.taps
        col, hist, mom = d.new_colour(), d.new_history(), d.new_moments()
        d.TemporalFilter(G.dev(t["prev_colour"]), G.dev(t["radiance"]), col, gbs[k], gbs[kp], G.dev(t["prev_hist"]), hist, mom, G.dev(t["prev_mom"]))
        assert np.array_equal(G.host(hist), t["hist"]), f"frame {k}: history"
        assert np.array_equal(G.host(col).view(np.uint8), t["temporal"].view(np.uint8)), f"frame {k}: temporal colour"
        assert np.array_equal(G.host(mom).view(np.uint8), t["mom"].view(np.uint8)), f"frame {k}: temporal moments"
        out = d.new_colour()
        d.FilterMoments(G.dev(t["temporal"]), out, G.dev(t["mom"]), gbs[k], G.dev(t["hist"]))
        assert np.abs(G.host(out).astype(np.float64) - t["moments"].astype(np.float64)).max() <= 8e-5, f"frame {k}: moments"
        for i in range(5):
            d.FilterKernel(G.dev(t["atrous_in"][i]), out, G.dev(t["temporal"]) if i == 0 else None, gbs[k], 1 << i, i)
            G.assert_colour_close(G.host(out), t["atrous_out"][i], storage, f"frame {k} a-trous step {1 << i}")
        want = hip.frame(fr[k]["radiance"], gbs[k], gbs[kp])
        got = drv.Render(G.dev(fr[k]["radiance"]), gbs[k], gbs[kp] if k else None)
        torch.cuda.synchronize()
        assert np.array_equal(G.host(got).view(np.uint8), want.view(np.uint8)), f"frame {k}: frame driver"
    assert 0 < int(cs.listed_young(t["hist"], fr[-1]["normal"]).sum()) < W4 * H4 // 4
    for x in (d, drv):
        x.close()


# ------------------------------------------------------------------ g
def _sentinel(shape, dtype):
    import torch
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(BYTE_SENTINEL)
    return t


def _pack(G, d, fr, sl, outs):
    """svgf_pack_gbuffer of context d on the attribute rows `sl`, into caller-filled planes."""
    from svgf_amd import filter as F
    cam = F.CameraC((C.c_float * 16)(*map(float, fr["vp"])), (C.c_float * 16)(*map(float, fr["prev_vp"])), (C.c_float * 3)(*map(float, fr["eye"])))
    planes = [G.dev(np.ascontiguousarray(fr[k][sl])) for k in ("position", "normal_in", "bary")]
    rc = d.lib.svgf_pack_gbuffer(d._h, *[F._ptr(p) for p in planes], C.byref(cam), *[F._ptr(o) for o in outs])
    return rc


@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_taa_and_adapter_on_strips_and_row_ranges(G, oracle, storage):
    import torch
    from svgf_amd import filter as F
    fr = _seq("orbit", 4)[3]
    dt = CDT[storage]
    rng = np.random.default_rng(11)
    filt = np.concatenate([fr["base"], np.ones((H, W, 1), np.float32)], -1).astype(dt)
    hist = rng.uniform(0, 1, (H, W, 4)).astype(dt)
    tdt = torch.float32 if storage == "f32" else torch.float16
    whole = F.Denoiser(W, H, F.Params(storage=storage))
    w_out = whole.new_colour()
    whole.TAA(G.dev(filt), G.dev(hist), w_out)
    w_taa = G.host(w_out)
    w_gb = [torch.empty((H, W, 4), dtype=t, device="cuda") for t in (torch.float32, torch.int16, torch.int16)]
    assert _pack(G, whole, fr, slice(0, H), w_gb) == 0
    w_pack = [G.host(t).view(np.uint8) for t in w_gb]
    assert np.array_equal(w_pack[0], fr["motion"].view(np.uint8))
    # strips (odd y0 and own rows among them) and row ranges of the whole-frame context
    for y0, rows in [(37, 101), (0, 60), (250, 83), (101, 50)]:
        for halo, ok in ((3, True), (2, False)):
            own0_, own1_ = y0 + halo if y0 > 0 else 0, (y0 + rows - halo) if y0 + rows < H else H
            s = F.Denoiser(W, H, F.Params(storage=storage), strip=(y0, rows, own0_, own1_))
            sl = slice(y0, y0 + rows)
            out = _sentinel((rows, W, 4), tdt)
            if not ok:
                with pytest.raises(F.SvgfError, match="halo"):
                    s.TAA(G.dev(np.ascontiguousarray(filt[sl])), G.dev(np.ascontiguousarray(hist[sl])), out)
                s.close()
                continue
            s.TAA(G.dev(np.ascontiguousarray(filt[sl])), G.dev(np.ascontiguousarray(hist[sl])), out)
            got = G.host(out)
            a, b = own0_ - y0, own1_ - y0
            assert np.array_equal(got[a:b].view(np.uint8), w_taa[own0_:own1_].view(np.uint8)), (y0, rows, "taa rows")
            assert np.all(got[:a].view(np.uint8) == BYTE_SENTINEL) and np.all(got[b:].view(np.uint8) == BYTE_SENTINEL), (y0, rows, "taa wrote outside its rows")
            want = np.zeros((rows, W, 4), dt)
            oracle.taa(W, H, storage, np.ascontiguousarray(filt[sl]), np.ascontiguousarray(hist[sl]), want, geo=(y0, rows, own0_, own1_))
            if storage == "f32":
                assert np.abs(got[a:b].astype(np.float64) - want[a:b].astype(np.float64)).max() <= 2e-6
            else:
                from tests.helpers import half_ulp_diff
                assert half_ulp_diff(got[a:b], want[a:b]).max() <= 1
            s.close()
        # the adapter: a halo of one row (its quad partner), refused with none
        for halo, ok in ((1, True), (0, False)):
            own0_, own1_ = y0 + halo if y0 > 0 else 0, (y0 + rows - halo) if y0 + rows < H else H
            s = F.Denoiser(W, H, F.Params(storage=storage), strip=(y0, rows, own0_, own1_))
            outs = [_sentinel((rows, W, 4), t) for t in (torch.float32, torch.int16, torch.int16)]
            rc = _pack(G, s, fr, slice(y0, y0 + rows), outs)
            torch.cuda.synchronize()
            if not ok:
                assert rc == -4, (y0, rows, rc)                   # SVGF_ERR_HALO
                s.close()
                continue
            assert rc == 0
            a, b = own0_ - y0, own1_ - y0
            for o, wp in zip(outs, w_pack):
                g8 = G.host(o).view(np.uint8)
                assert np.array_equal(g8[a:b], wp[own0_:own1_]), (y0, rows, "adapter rows")
                assert np.all(g8[:a] == BYTE_SENTINEL) and np.all(g8[b:] == BYTE_SENTINEL), (y0, rows, "the adapter wrote outside its rows")
            s.close()
    # row ranges of the whole-frame context (svgf_set_rows), odd first rows
    for rb, re in [(0, 1), (33, 97), (101, 102), (250, 333)]:
        whole.set_rows(rb, re)
        out = _sentinel((H, W, 4), tdt)
        whole.TAA(G.dev(filt), G.dev(hist), out)
        got = G.host(out).view(np.uint8)
        assert np.array_equal(got[rb:re], w_taa.view(np.uint8)[rb:re]) and np.all(got[:rb] == BYTE_SENTINEL) and np.all(got[re:] == BYTE_SENTINEL), (rb, re, "taa")
        outs = [_sentinel((H, W, 4), t) for t in (torch.float32, torch.int16, torch.int16)]
        assert _pack(G, whole, fr, slice(0, H), outs) == 0
        for o, wp in zip(outs, w_pack):
            g8 = G.host(o).view(np.uint8)
            assert np.array_equal(g8[rb:re], wp[rb:re]) and np.all(g8[:rb] == BYTE_SENTINEL) and np.all(g8[re:] == BYTE_SENTINEL), (rb, re, "adapter")
    whole.set_rows()
    whole.close()


# ------------------------------------------------------------------ h
def _build_seq_exe():
    from svgf_amd import build as b
    from tests.conftest import ROOT
    b.build_library()
    exe = os.path.join(ROOT, "tests", "cpp", "shim_sequence")
    cmd = ["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
           os.path.join(ROOT, "tests", "cpp", "shim_sequence.cpp"), "-o", exe, "-L", os.path.join(ROOT, "svgf_amd"), "-lsvgf_mi355x",
           "-L", "/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + os.path.join(ROOT, "svgf_amd"), "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_cpp_drop_in_over_a_camera_path(G, oracle, tmp_path, storage):
    """gpupt::svgfDenoiser over the dolly with distinct current and previous G-buffers: every frame's result bit-identical to the stage calls
    (gpu_helpers.HipPipeline), every frame's history equal to the oracle's."""
    exe = _build_seq_exe()
    N = 6
    fr = _seq("dolly", N)
    for k, f in enumerate(fr):
        for name in ("motion", "normal", "uv"):
            np.ascontiguousarray(f[name]).tofile(tmp_path / f"{name}_{k}.bin")
        np.ascontiguousarray(f["radiance"].astype(CDT[storage])).tofile(tmp_path / f"radiance_{k}.bin")
    r = subprocess.run([exe, str(tmp_path), str(W), str(H), str(N), "1" if storage == "f16" else "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "sequence ok" in r.stdout, r.stdout + r.stderr
    hip = G.HipPipeline(W, H, storage, steps=5)
    ref = oracle.Pipeline(W, H, storage, steps=5, nthreads=NT)
    gbs = [G.gb_dev(f) for f in fr]
    dt = CDT[storage]
    for k in range(N):
        kp = max(k - 1, 0)
        want = hip.frame(fr[k]["radiance"], gbs[k], gbs[kp])
        ref.frame(fr[k]["radiance"], gbuf(fr[k]), gbuf(fr[kp]))
        got = np.fromfile(tmp_path / f"out_{k}.bin", dt).reshape(H, W, 4)
        hist = np.fromfile(tmp_path / f"hist_{k}.bin", np.uint8).reshape(H, W)
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), f"frame {k}: result"
        assert np.array_equal(hist, ref.taps["hist"]), f"frame {k}: history"
    assert 0 < (hist > 1).mean() < 1
