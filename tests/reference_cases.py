"""The cases in which the CPU oracle is held to the reference's own filter source (oracle/ref_harness.cpp: Filter.cuh compiled for the host
against the stand-in headers of oracle/ref_shim/), shared by
  tests/test_reference_parity.py        oracle against the live reference build, and against the recorded fixtures
  tests/golden/make_golden.py           records the reference build's outputs (tests/golden/ref_*.npz)
  tests/test_gpu_reference_fixtures.py  the HIP kernels against the recorded outputs.
Inputs are made here from seeds (svgf_amd.synth, tests/camera_scene.py, numpy Generators): a fixture stores outputs and parameters, never inputs.
fp16 storage throughout: the reference has no other (its kernels take half4* / half2*).

Every stage has a `Side`: the same call on the oracle or on the reference build, with the reference's in-place buffers (the radiance plane that
becomes the temporal output, the single history plane, the TAA output that is its own history) unfolded into the oracle's separate planes."""
from __future__ import annotations

import numpy as np

from svgf_amd import synth
from tests.gbuffer_poison import poison_gbuffer
from tests.helpers import gbuf

F16 = np.float16
SIZES = ((64, 48), (37, 29))
DEFAULT_THRESHOLDS = (0.8, 0.9)                # src/App.h:110-111
OTHER_THRESHOLDS = (0.05, 0.995)
MOTIONS = ((0.0, 0.0), (1.0, 0.0), (-2.5, 1.5))
SEQUENCE = dict(frames=6, steps=5, mv=(-2.5, 1.5))


# ------------------------------------------------------------------------------------------------------------------------------ sides
class OracleSide:
    """The stages on oracle/svgf_oracle.cpp (flavour: "oracle", or an envelope build such as "fma")."""
    name = "oracle"

    def __init__(self, orc, flavour="oracle"):
        self.orc, self.flavour = orc, flavour

    def temporal(self, W, H, prev_colour, radiance, gb_cur, gb_prev, hist_prev, mom_prev, *, depth_threshold, normal_threshold, history_base, mesh_id_test):
        out, hist, mom = np.zeros((H, W, 4), F16), np.zeros((H, W), np.uint8), np.zeros((H, W, 2), F16)
        with self.orc.using(self.flavour):
            self.orc.temporal(W, H, "f16", prev_colour, radiance, out, gb_cur, gb_prev, hist_prev, hist, mom, mom_prev, depth_threshold=depth_threshold,
                              normal_threshold=normal_threshold, history_base=history_base, mesh_id_test=mesh_id_test)
        return out, hist, mom

    def moments(self, W, H, colour, mom, gb, hist, *, phi_colour, phi_normal):
        out = np.zeros((H, W, 4), F16)
        with self.orc.using(self.flavour):
            self.orc.moments(W, H, "f16", colour, out, mom, gb, hist, phi_colour=phi_colour, phi_normal=phi_normal, radius=3)
        return out

    def atrous(self, W, H, src, feedback, gb, hist, *, step, phi_colour, phi_normal, iteration):
        """-> (output, feedback plane after the launch); `feedback` (copied) is RenderOutput's previous contents, or None"""
        out = np.zeros((H, W, 4), F16)
        fb = None if feedback is None else feedback.copy()
        with self.orc.using(self.flavour):
            self.orc.atrous(W, H, "f16", src, out, fb if iteration == 0 else None, gb, step=step, phi_colour=phi_colour, phi_normal=phi_normal, iteration=iteration)
        return out, fb

    def taa(self, W, H, filtered, history):
        out = np.zeros((H, W, 4), F16)
        with self.orc.using(self.flavour):
            self.orc.taa(W, H, "f16", filtered, history, out)
        return out

    def srgb(self, plane):
        """{ToSRGB(rgb), 1} of a float32 (H, W, 4) plane: what TonemapKernel stores"""
        out = np.ones_like(plane)
        with self.orc.using(self.flavour):
            out[..., :3] = self.orc.srgb(plane[..., :3])
        return out


class ReferenceSide:
    """The same stages on the host build of the reference's Filter.cuh (fma: the -ffp-contract=fast twin)."""
    name = "reference"

    def __init__(self, orc, fma=False):
        self.orc, self.fma = orc, fma

    def temporal(self, W, H, prev_colour, radiance, gb_cur, gb_prev, hist_prev, mom_prev, *, depth_threshold, normal_threshold, history_base, mesh_id_test):
        colour, hist, mom = radiance.copy(), hist_prev.copy(), np.zeros((H, W, 2), F16)       # in place: CurrentImage, HistoryLengths
        self.orc.ref_temporal(W, H, prev_colour, colour, gb_cur, gb_prev, hist, mom, mom_prev, depth_threshold=depth_threshold,
                              normal_threshold=normal_threshold, history_base=history_base,
                              uv_fetch=self.orc.UV_FETCH_AS_HALF if mesh_id_test else self.orc.UV_FETCH_RAW_BITS, fma=self.fma)
        return colour, hist, mom

    def moments(self, W, H, colour, mom, gb, hist, *, phi_colour, phi_normal):
        out = np.zeros((H, W, 4), F16)
        self.orc.ref_moments(W, H, colour, out, mom, gb, hist, phi_colour=phi_colour, phi_normal=phi_normal, fma=self.fma)
        return out

    def atrous(self, W, H, src, feedback, gb, hist, *, step, phi_colour, phi_normal, iteration):
        out = np.zeros((H, W, 4), F16)
        fb = None if feedback is None else feedback.copy()
        self.orc.ref_atrous(W, H, src, out, fb if iteration == 0 else None, gb, hist, step=step, phi_colour=phi_colour, phi_normal=phi_normal,
                            iteration=iteration, fma=self.fma)
        return out, fb

    def taa(self, W, H, filtered, history):
        out = history.copy()                                                                  # in place: Output is its own history
        self.orc.ref_taa(W, H, filtered, out, fma=self.fma)
        return out

    def srgb(self, plane):
        H, W = plane.shape[:2]
        out = np.zeros_like(plane)
        self.orc.ref_tonemap(W, H, np.ascontiguousarray(plane), out, fma=self.fma)
        return out


# ------------------------------------------------------------------------------------------------------------------------------ inputs
def _sprinkle(rng, plane, n):
    """n texels (single channels) of NaN / +inf / -inf / -0.0 into a float plane, as the `stage` sweep of tests/fuzz_parity.py plants them"""
    flat = plane.reshape(-1)
    idx = rng.choice(flat.size, n, replace=False)
    flat[idx] = rng.choice(np.array([np.nan, np.inf, -np.inf, -0.0], np.float32), n).astype(plane.dtype)


def frame_pair(W, H, mv=(-2.5, 1.5), camera=False, poison=False, seed=0):
    """-> (previous frame, current frame): synth.make_frame 0 and 1 under `mv`, or frames 2 and 3 of tests/camera_scene.py's orbit"""
    if camera:
        from tests import camera_scene
        f0, f1 = camera_scene.make_frame("orbit", 2, W, H), camera_scene.make_frame("orbit", 3, W, H)
    else:
        f0, f1 = synth.make_frame(W, H, 0, mv=mv), synth.make_frame(W, H, 1, mv=mv)
    if poison:
        rng = np.random.default_rng(1000 + seed)
        what = ("motion", "depth", "ddepth", "normal", "id")
        f0, f1 = poison_gbuffer(rng, f0, what, per_value=2)[0], poison_gbuffer(rng, f1, what, per_value=2)[0]
    return f0, f1


def temporal_inputs(W, H, f1, seed=0, poison=False):
    """previous colour (beyond [0,1] on both sides: the value clamp), radiance, previous history over 0..255, previous moments"""
    rng = np.random.default_rng(2000 + seed)
    prev = np.concatenate([rng.uniform(-0.2, 1.3, (H, W, 3)), rng.uniform(-0.01, 0.2, (H, W, 1))], -1).astype(F16)
    rad = np.ascontiguousarray(f1["radiance"].astype(F16))
    hist = rng.permutation(np.arange(W * H) % 256).astype(np.uint8).reshape(H, W)
    mom = rng.uniform(0.0, 1.0, (H, W, 2)).astype(F16)
    if poison:
        _sprinkle(rng, prev, 24); _sprinkle(rng, rad, 24); _sprinkle(rng, mom, 12)
    return prev, rad, hist, mom


def spatial_inputs(W, H, seed=0, poison=False, hist_max=8):
    """colour {rgb beyond [0,1], variance around 0}, moments, history 0..hist_max-1 (both branches of FilterMoments), marker-filled feedback plane"""
    rng = np.random.default_rng(3000 + seed)
    src = np.concatenate([rng.uniform(-0.2, 1.3, (H, W, 3)), rng.uniform(-0.01, 0.2, (H, W, 1))], -1).astype(F16)
    mom = rng.uniform(0.0, 1.0, (H, W, 2)).astype(F16)
    hist = rng.integers(0, hist_max, (H, W)).astype(np.uint8)
    marker = np.full((H, W, 4), 7.0, F16)
    if poison:
        _sprinkle(rng, src, 32); _sprinkle(rng, mom, 12)
    return src, mom, hist, marker


def taa_inputs(W, H, seed=0, poison=False):
    rng = np.random.default_rng(4000 + seed)
    filt = np.concatenate([rng.uniform(-0.2, 1.3, (H, W, 3)), rng.uniform(-0.01, 0.2, (H, W, 1))], -1).astype(F16)
    hist = rng.uniform(-0.1, 1.1, (H, W, 4)).astype(F16)
    hist[::3, ::2, 3] = 0.0                     # a mix rate of 0 (an untouched history plane) next to 1 and everything between
    if poison:
        _sprinkle(rng, filt, 32); _sprinkle(rng, hist, 32)
    return filt, hist


def tonemap_input(W, H, seed=0, poison=False):
    rng = np.random.default_rng(5000 + seed)
    a = rng.uniform(-0.1, 1.5, (H, W, 4)).astype(np.float32)
    a[::2, ::3, :3] *= np.float32(0.004)        # both branches of ToSRGB (the knee is at 0.0031308)
    if poison:
        _sprinkle(rng, a, 32)
    return a


def accept_mask(side, W, H, rad, gb1, gb0, hist, mom, **kw):
    """Which texels TemporalFilter accepted (LoadPreviousData returned true), made observable: with a previous colour of NaN everywhere (imageLoad's
    clamp is built from comparisons and passes a NaN; an infinity it would clamp to 1) an accepted texel blends in NaN * (1 - a), a NaN even when
    a = 1, and a rejected one blends in the zero it starts from.  (The radiance's own non-finite texels are taken out first.)"""
    probe = np.full((H, W, 4), np.nan, F16)
    clean = np.nan_to_num(rad.astype(np.float32), nan=0.0, posinf=1.0, neginf=0.0).astype(F16)
    out, _, _ = side.temporal(W, H, probe, clean, gb1, gb0, hist, mom, **kw)
    return np.isnan(out[..., 0].astype(np.float32))


# ------------------------------------------------------------------------------------------------------------------------------ sequence
def oracle_sequence(orc, W, H, flavour="oracle", frames=SEQUENCE["frames"], steps=SEQUENCE["steps"], mv=SEQUENCE["mv"]):
    """-> per frame dict(colour, mom, hist, out): the state planes of oracle.Pipeline after the frame, and its output"""
    p = orc.Pipeline(W, H, "f16", steps=steps)
    fr = [synth.make_frame(W, H, k, mv=mv) for k in range(frames)]
    got = []
    for k in range(frames):
        with orc.using(flavour):
            out = p.frame(fr[k]["radiance"], gbuf(fr[k]), gbuf(fr[max(k - 1, 0)]))
        P = p.P ^ 1
        got.append(dict(colour=p.colour[P].copy(), mom=p.mom[P].copy(), hist=p.hist[P].copy(), out=out.copy()))
    return got


def reference_sequence(orc, W, H, fma=False, frames=SEQUENCE["frames"], steps=SEQUENCE["steps"], mv=SEQUENCE["mv"]):
    """The reference's kernels in the order and ping-pong of its host code, restated (App.cu is not compiled):
        App.cu:552-556   per frame: TemporalFilter(); FilterMoments(); WaveletFilter(); then PingPongInx = 1 - PingPongInx
        App.cu:473-477   TemporalFilter(RenderBuffer[1-P], RenderBuffer[P] in place, Framebuffer[P], Framebuffer[1-P], HistoryLengthBuffer,
                                        MomentsBuffer[P], MomentsBuffer[1-P])
        App.cu:484-488   FilterMoments(RenderBuffer[P] -> FilterBuffer[0], MomentsBuffer, Framebuffer[P], HistoryLengthBuffer)
        App.cu:496-507   for i < steps: FilterKernel(FilterBuffer[pp] -> FilterBuffer[1-pp], RenderOutput = RenderBuffer[P], step 1 << i, iteration i); pp = 1 - pp
        App.cu:510-513   odd step count: FilterBuffer[1] copied to FilterBuffer[0]
    with the host-side decisions of SURVEY.md App. B that this project made, none of which is kernel text: #4 FilterMoments is handed the CURRENT
    moments, MomentsBuffer[P] (the reference hands it MomentsBuffer[0]); #9 every buffer starts zeroed; and the path tracer's write of
    RenderBuffer[P] is the synthetic radiance.  The single HistoryLengthBuffer is the reference's (the harness gives its in-place launch
    snapshot semantics, App. B #1)."""
    z4 = lambda: np.zeros((H, W, 4), F16)                                                     # noqa: E731
    render, filt, mom = [z4(), z4()], [z4(), z4()], [np.zeros((H, W, 2), F16) for _ in range(2)]
    hist = np.zeros((H, W), np.uint8)
    P = 0
    fr = [synth.make_frame(W, H, k, mv=mv) for k in range(frames)]
    got = []
    for k in range(frames):
        gb_c, gb_p = gbuf(fr[k]), gbuf(fr[max(k - 1, 0)])
        render[P][...] = fr[k]["radiance"].astype(F16)                                        # Trace()
        orc.ref_temporal(W, H, render[1 - P], render[P], gb_c, gb_p, hist, mom[P], mom[1 - P], depth_threshold=orc.DEFAULTS["depth_threshold"],
                         normal_threshold=orc.DEFAULTS["normal_threshold"], history_base=orc.DEFAULTS["history_base"], fma=fma)
        orc.ref_moments(W, H, render[P], filt[0], mom[P], gb_c, hist, phi_colour=orc.DEFAULTS["phi_colour"], phi_normal=orc.DEFAULTS["phi_normal"], fma=fma)
        pp = 0
        for i in range(steps):
            orc.ref_atrous(W, H, filt[pp], filt[1 - pp], render[P], gb_c, hist, step=1 << i, phi_colour=orc.DEFAULTS["phi_colour"],
                           phi_normal=orc.DEFAULTS["phi_normal"], iteration=i, fma=fma)
            pp = 1 - pp
        if steps % 2:
            filt[0][...] = filt[1]
        got.append(dict(colour=render[P].copy(), mom=mom[P].copy(), hist=hist.copy(), out=filt[0].copy()))
        P = 1 - P
    return got


# ------------------------------------------------------------------------------------------------------------------------------ comparing
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def same_bits(got, want):
    """-> boolean array: bit for bit the same — the sign of a zero and every infinity included — except that a NaN is a NaN: its payload and sign are
    the converter's (cvt.rn.f16.f32 makes 0x7fff, vcvtps2ph and the oracle's converter keep the sign) and are not compared."""
    if got.dtype.kind != "f":
        return got == want
    gn, wn = np.isnan(got), np.isnan(want)
    return (gn & wn) | (~gn & ~wn & (bits(got) == bits(want)))


def differing(got, want):
    return int((~same_bits(got, want)).sum())


# ------------------------------------------------------------------------------------------------------------------------------ fixtures
# What tests/golden/ref_stages_64x48.npz and ref_sequence_64x48.npz record: the reference build's OUTPUTS for a subset of the cases above, next
# to the parameters that regenerate the inputs here.  fixture_inputs() is the one place that turns those parameters into planes.
FIXTURE_SIZE = (64, 48)
FIXTURE_PARAMS = dict(W=64, H=48, mv=np.array([-2.5, 1.5]), seed=0, depth_threshold=0.8, normal_threshold=0.9, history_base=24, mesh_id_test=1,
                      phi_colour=10.0, phi_normal=128.0, atrous=np.array([[1, 0], [4, 1]]),          # (step, iteration)
                      sequence_frames=SEQUENCE["frames"], sequence_steps=SEQUENCE["steps"])


def fixture_inputs(params=FIXTURE_PARAMS):
    """-> dict: the frame pair and every stage's input planes, clean and (spatial stages) poisoned, from the parameters a fixture stores"""
    W, H, seed = int(params["W"]), int(params["H"]), int(params["seed"])
    mv = tuple(float(v) for v in params["mv"])
    f0, f1 = frame_pair(W, H, mv=mv)
    p0, p1 = frame_pair(W, H, mv=mv, poison=True, seed=seed)
    return dict(W=W, H=H, f0=f0, f1=f1, temporal=temporal_inputs(W, H, f1, seed=seed), spatial=spatial_inputs(W, H, seed=seed),
                p1=p1, spatial_poison=spatial_inputs(W, H, seed=seed, poison=True), taa=taa_inputs(W, H, seed=seed))


def fixture_stage_outputs(side, params=FIXTURE_PARAMS):
    """-> dict name -> plane: what `side` computes for the fixture's stage cases"""
    i = fixture_inputs(params)
    W, H = i["W"], i["H"]
    phi = dict(phi_colour=float(params["phi_colour"]), phi_normal=float(params["phi_normal"]))
    out = {}
    prev, rad, hist, mom = i["temporal"]
    out["temporal_colour"], out["temporal_hist"], out["temporal_mom"] = side.temporal(
        W, H, prev, rad, gbuf(i["f1"]), gbuf(i["f0"]), hist, mom, depth_threshold=float(params["depth_threshold"]),
        normal_threshold=float(params["normal_threshold"]), history_base=int(params["history_base"]), mesh_id_test=int(params["mesh_id_test"]))
    for tag, (src, mom, hist, marker), f in (("", i["spatial"], i["f1"]), ("_poison", i["spatial_poison"], i["p1"])):
        out["moments" + tag] = side.moments(W, H, src, mom, gbuf(f), hist, **phi)
        for step, iteration in (tuple(int(v) for v in row) for row in params["atrous"]):
            if tag and iteration:
                continue                                   # (poisoned: iteration 0 only — the result, the feedback and the sky copy in one launch)
            o, fb = side.atrous(W, H, src, marker, gbuf(f), hist, step=step, iteration=iteration, **phi)
            out[f"atrous_step{step}_it{iteration}{tag}"] = o
            if iteration == 0:
                out[f"atrous_step{step}_it{iteration}{tag}_feedback"] = fb
    out["taa"] = side.taa(W, H, *i["taa"])
    return out


def fixture_sequence_outputs(frames):
    """-> dict: the final plane and history (and the state the next frame would read) of a six-frame sequence (oracle_sequence / reference_sequence)"""
    last = frames[-1]
    return dict(out=last["out"], hist=last["hist"], colour=last["colour"], mom=last["mom"])
