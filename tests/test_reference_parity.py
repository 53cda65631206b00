"""The CPU oracle against the reference's OWN filter source.

oracle/svgf_oracle.cpp is where every parity claim of this project ends, and it was written by this project — as was its NumPy twin, from the same
reading of the reference's Filter.cuh.  Here it is held to that file itself: __graft_entry__.build() copies Filter.cuh, unmodified, next to
oracle/ref_harness.cpp and compiles it for the host against the stand-in headers of oracle/ref_shim/ (glm, the CUDA overload sets, cvt.rzi,
F16C half conversions, point-sampled textures), and the harness runs its kernels thread by thread (oracle/_ref/libsvgf_ref.so).

Live part (needs oracle/_ref): every stage on 64x48 and 37x29 frames, fp16 storage (the reference has no other), bit for bit — the sign of a zero
and every infinity included, a NaN being a NaN whatever its payload (tests/reference_cases.py: same_bits).  Where the reference checkout exists
and the library does not, these tests FAIL: they do not skip.  Fixture part (always on): the oracle against the reference build's recorded
outputs, tests/golden/ref_*.npz, held the same way.

Agreement reached (also DESIGN.md §4), on the build with the oracle's flags (-O2 -ffp-contract=off):
    temporal (colour, moments, history, accept mask), moments, à-trous (result, feedback, sky copy), TAA, tonemap, the six-frame sequence:
    BIT-EXACT on every case below, poisoned input included.  No texel is excluded under any item of SURVEY.md App. B (cap: 1 % per case; used: 0).
The -ffp-contract=fast twin (libsvgf_ref_fma.so against libsvgf_oracle_fma.so) is a different matter: where a compiler contracts a*b+c depends
on how the source spells the expression, so two sources of the same arithmetic are two draws of that freedom.  Temporal, moments and tonemap are
bit-exact there too; à-trous, TAA and the sequence differ on a few values.  They are bounded not by a tolerance but CASE BY CASE (one launch, or
one plane of one frame of the sequence): every value of reference_fma is within twice the distance the oracle keeps from ITS OWN fma build in that
same case (what DESIGN.md §4 treats as "other correct builds"; x2 because that distance is one draw and the reference's twin another) — or within
one half-ulp of oracle_fma.  The floor is the number format's, not a measurement: one fp32 rounding placed differently can move a result across a
half rounding boundary wherever that lies, whether or not the oracle's own pair happened to cross one in that case.  Measured, largest residual
(reference_fma <-> oracle_fma) against that case's envelope (oracle <-> oracle_fma): à-trous 3.1e-5 / 3.1e-5 (64x48) and 3.8e-6 / 3.8e-6 (37x29),
both one half-ulp; TAA 1.2e-4 / 2.7e-4 and 9.2e-5 / 1.2e-4; sequence, worst plane (frame 3 output) 2.4e-4 / 2.4e-4.  No value is beyond both.
NaN masks, infinities, history and accept masks are exact in the twin as well."""
import itertools
import os

import numpy as np
import pytest

from svgf_amd import synth
from tests import reference_cases as rc
from tests.conftest import ROOT
from tests.helpers import gbuf

GOLD = os.path.join(ROOT, "tests", "golden")
PHI = [(pc, pn) for pc in (10.0, 0.05, 100.0) for pn in (128.0, 0.5)]
ENVELOPE_MARGIN = 2.0


@pytest.fixture(scope="module")
def ref(oracle):
    """The live reference build.  Present: returned.  Absent although the reference checkout is there: the test FAILS (build() makes it).
    Absent with no reference checkout: only then is there nothing to run against (the fixture tests below stand in)."""
    lib = os.path.join(ROOT, "oracle", "_ref", "libsvgf_ref.so")
    if not os.path.exists(lib):
        if oracle.reference_available():
            pytest.fail(f"{lib} is missing although the reference checkout is at {oracle.REFERENCE_DIR}: __graft_entry__.build() builds it")
        pytest.skip("no reference checkout and no oracle/_ref on this machine: the recorded fixtures stand in")
    here = os.path.join(ROOT, "oracle")
    srcs = [os.path.join(here, "ref_harness.cpp")] + [os.path.join(dp, f) for dp, _, fs in os.walk(os.path.join(here, "ref_shim")) for f in fs]
    assert os.path.getmtime(lib) >= max(os.path.getmtime(s) for s in srcs), "oracle/_ref is older than its sources: run __graft_entry__.build()"
    oracle.ref_lib(False)
    return oracle


def exact(got, want, what):
    bad = ~rc.same_bits(got, want)
    assert not bad.any(), f"{what}: {int(bad.sum())} values differ from the reference; first at {np.argwhere(bad)[:4].tolist()}"


def dist(a, b):
    """max |a - b| over the finite values; NaN masks and infinities must already agree"""
    a, b = a.astype(np.float64), b.astype(np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b)) and np.array_equal(a[np.isinf(a)], b[np.isinf(b)])
    fin = np.isfinite(a)
    return float(np.abs(a[fin] - b[fin]).max()) if fin.any() else 0.0


def twin_case(o, of, rf, what):
    """One case of the -ffp-contract=fast pair: o = oracle, of = oracle_fma, rf = reference_fma.  Every value of rf is within ENVELOPE_MARGIN x this
    case's envelope max |o - of| of its value in of, or within one half-ulp of it (module docstring).  -> (residual, envelope)"""
    from tests.helpers import half_ulp_diff
    envelope, residual = dist(o, of), dist(rf, of)
    fin = np.isfinite(of.astype(np.float32))
    beyond = np.abs(rf[fin].astype(np.float64) - of[fin].astype(np.float64)) > ENVELOPE_MARGIN * envelope
    flips = half_ulp_diff(rf[fin], of[fin]) if rf.dtype == np.float16 else np.where(rf[fin] == of[fin], 0, 2)
    bad = int((beyond & (flips > 1)).sum())
    assert bad == 0, f"{what}: {bad} values of reference_fma are beyond {ENVELOPE_MARGIN} x {envelope:.3e} (oracle <-> oracle_fma, this case) and one half-ulp from oracle_fma; residual {residual:.3e}"
    return residual, envelope


def fma_or_skip(orc):
    try:
        orc.lib("fma")
        orc.ref_lib(True)
    except orc.EnvelopeUnavailable as e:
        pytest.skip(str(e))


# ------------------------------------------------------------------------------------------------------------------------------ live
TEMPORAL_INPUTS = [("mv0", dict(mv=(0.0, 0.0))), ("mv1", dict(mv=(1.0, 0.0))), ("mv-2.5_1.5", dict(mv=(-2.5, 1.5))), ("camera", dict(camera=True))]


@pytest.mark.parametrize("poison", [False, True], ids=["clean", "poisoned"])
@pytest.mark.parametrize("inputs", TEMPORAL_INPUTS, ids=[n for n, _ in TEMPORAL_INPUTS])
@pytest.mark.parametrize("size", rc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_temporal(ref, size, inputs, poison):
    """TemporalFilter + LoadPreviousData (Filter.cuh:225-258,359-404): uniform motion (0,0), (1,0), (-2.5,1.5) — truncation toward zero of a negative
    vector — and per-pixel motion from a moving camera; previous history over 0..255; history_base 1, 24, 255; the default thresholds and another
    pair; both readings of the UV fetch of :245-246 (raw bits = the oracle's mesh_id_test 0, halves = 1).  Poisoned: tests/gbuffer_poison.py on both
    G-buffers plus NaN / +-inf / -0.0 texels in the colour and moments planes — where the stand-ins' overload and conversion rules decide."""
    (W, H), kw = size, inputs[1]
    f0, f1 = rc.frame_pair(W, H, poison=poison, **kw)
    prev, rad, hist, mom = rc.temporal_inputs(W, H, f1, poison=poison)
    assert len(np.unique(hist)) == 256
    O, R = rc.OracleSide(ref), rc.ReferenceSide(ref)
    accepted = []
    for base, thr, mid in itertools.product((1, 24, 255), (rc.DEFAULT_THRESHOLDS, rc.OTHER_THRESHOLDS), (0, 1)):
        p = dict(depth_threshold=thr[0], normal_threshold=thr[1], history_base=base, mesh_id_test=mid)
        what = f"temporal {W}x{H} {inputs[0]} base {base} thresholds {thr} uv fetch {mid}"
        for name, a, b in zip(("colour", "history", "moments"), O.temporal(W, H, prev, rad, gbuf(f1), gbuf(f0), hist, mom, **p),
                              R.temporal(W, H, prev, rad, gbuf(f1), gbuf(f0), hist, mom, **p)):
            exact(a, b, f"{what}: {name}")
        ma, mb = (rc.accept_mask(s, W, H, rad, gbuf(f1), gbuf(f0), hist, mom, **p) for s in (O, R))
        assert np.array_equal(ma, mb), f"{what}: accept masks differ at {np.argwhere(ma != mb)[:4].tolist()}"
        assert 0.0 < ma.mean() < 1.0, f"{what}: the case must hold accepted and rejected texels"
        accepted.append(float(ma.mean()))
    assert max(accepted) > 0.2


@pytest.mark.parametrize("poison", [False, True], ids=["clean", "poisoned"])
@pytest.mark.parametrize("size", rc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_moments(ref, size, poison):
    """FilterMoments (Filter.cuh:430-525): radius 3 — the reference has no other; history 0..7, so both branches run; raw (unclamped) loads and stores."""
    W, H = size
    _, f1 = rc.frame_pair(W, H, poison=poison)
    src, mom, hist, _ = rc.spatial_inputs(W, H, poison=poison)
    assert (hist < 4).any() and (hist >= 4).any() and (f1["region"] == synth.SKY).any()
    for pc, pn in PHI:
        a, b = (s.moments(W, H, src, mom, gbuf(f1), hist, phi_colour=pc, phi_normal=pn) for s in (rc.OracleSide(ref), rc.ReferenceSide(ref)))
        exact(a, b, f"moments {W}x{H} phi {pc}/{pn}")


@pytest.mark.parametrize("poison", [False, True], ids=["clean", "poisoned"])
@pytest.mark.parametrize("step", [1, 2, 4, 16])
@pytest.mark.parametrize("size", rc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_atrous(ref, size, step, poison):
    """FilterKernel (Filter.cuh:527-624): iteration 0 with RenderOutput and iteration 1 without; PhiColour 10, 0.05, 100; PhiNormal 128, 0.5; sky texels
    present — their copy (:554-558) and the texels that receive feedback (:619-622: a marker-filled plane keeps its marker on the sky) bit for bit."""
    W, H = size
    _, f1 = rc.frame_pair(W, H, poison=poison)
    src, _, hist, marker = rc.spatial_inputs(W, H, poison=poison)
    sky = (f1["motion"][..., 2] == 0) | (f1["motion"][..., 2] == np.float32(1e30))      # GetDepth's sentinel (:204), and a depth that equals it (:554)
    assert sky.any() and not sky.all()
    for (pc, pn), it in itertools.product(PHI, (0, 1)):
        (a, fa), (b, fb) = (s.atrous(W, H, src, marker, gbuf(f1), hist, step=step, phi_colour=pc, phi_normal=pn, iteration=it)
                            for s in (rc.OracleSide(ref), rc.ReferenceSide(ref)))
        what = f"a-trous {W}x{H} step {step} iteration {it} phi {pc}/{pn}"
        exact(a, b, what)
        exact(fa, fb, what + ": feedback")
        kept = (rc.bits(fb) == rc.bits(marker)).all(-1)
        assert np.array_equal(kept, sky if it == 0 else np.ones_like(sky)), what + ": which texels receive feedback"


@pytest.mark.parametrize("poison", [False, True], ids=["clean", "poisoned"])
@pytest.mark.parametrize("size", rc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_taa_and_tonemap(ref, size, poison):
    """TAAFilterKernel (Filter.cuh:288-357) against oracle.taa, TonemapKernel (:159-175) against the oracle's sRGB (:145-148)."""
    W, H = size
    O, R = rc.OracleSide(ref), rc.ReferenceSide(ref)
    filt, hist = rc.taa_inputs(W, H, poison=poison)
    exact(O.taa(W, H, filt, hist), R.taa(W, H, filt, hist), f"TAA {W}x{H}")
    t = rc.tonemap_input(W, H, poison=poison)
    assert (t[..., :3] <= 0.0031308).any() and (t[..., :3] > 0.0031308).any()
    exact(O.srgb(t), R.srgb(t), f"tonemap {W}x{H}")


@pytest.mark.parametrize("size", rc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sequence(ref, size):
    """Six frames, five iterations, motion (-2.5, 1.5): the reference's kernels in the order and ping-pong of App.cu:469-507,552-556 (restated in
    tests/reference_cases.py: reference_sequence) against oracle.Pipeline — every state plane after every frame."""
    W, H = size
    for k, (a, b) in enumerate(zip(rc.oracle_sequence(ref, W, H), rc.reference_sequence(ref, W, H))):
        for plane in ("colour", "mom", "hist", "out"):
            exact(a[plane], b[plane], f"sequence {W}x{H} frame {k}: {plane}")
    assert a["hist"].max() == 6 and (a["hist"] == 1).any()


def test_runner_reports_a_store_outside_the_threads_own_pixel(ref):
    """The harness's claim that a thread stored nowhere but at its own pixel, on a kernel of the harness's own that does: a stray store is reported
    (-2) whether it hits a pixel whose thread runs later (which would otherwise overwrite it) or earlier, inside the block or across the frame —
    and is undone, so the plane still holds every thread's own store and nothing else."""
    W, H = 37, 29
    rc0, plane = ref.ref_guard_selftest(W, H, 5, 5, 0, 0)
    assert rc0 == 0 and (plane == 1).all()
    for dx, dy in ((1, 0), (-1, 0), (1, 2), (-3, -2), (31, 23), (-5, -5)):
        rc_, plane = ref.ref_guard_selftest(W, H, 5, 5, dx, dy)
        assert rc_ == -2 and (plane == 1).all(), (dx, dy)


@pytest.mark.parametrize("size", rc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fma_twin_exact_stages(ref, size):
    """libsvgf_ref_fma.so against libsvgf_oracle_fma.so: temporal, moments and tonemap are bit-exact in the twin too."""
    fma_or_skip(ref)
    W, H = size
    OF, RF = rc.OracleSide(ref, "fma"), rc.ReferenceSide(ref, fma=True)
    for poison in (False, True):
        f0, f1 = rc.frame_pair(W, H, poison=poison)
        prev, rad, hist, mom = rc.temporal_inputs(W, H, f1, poison=poison)
        for mid in (0, 1):
            p = dict(depth_threshold=0.8, normal_threshold=0.9, history_base=24, mesh_id_test=mid)
            for a, b in zip(OF.temporal(W, H, prev, rad, gbuf(f1), gbuf(f0), hist, mom, **p), RF.temporal(W, H, prev, rad, gbuf(f1), gbuf(f0), hist, mom, **p)):
                exact(a, b, f"fma twin temporal {W}x{H}")
        src, mom, hist, _ = rc.spatial_inputs(W, H, poison=poison)
        exact(OF.moments(W, H, src, mom, gbuf(f1), hist, phi_colour=10.0, phi_normal=128.0), RF.moments(W, H, src, mom, gbuf(f1), hist, phi_colour=10.0, phi_normal=128.0),
              f"fma twin moments {W}x{H}")
        t = rc.tonemap_input(W, H, poison=poison)
        exact(OF.srgb(t), RF.srgb(t), f"fma twin tonemap {W}x{H}")


@pytest.mark.parametrize("step", [1, 2, 4, 16])
@pytest.mark.parametrize("size", rc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fma_twin_atrous_and_taa(ref, size, step):
    """The twin's à-trous (both iterations, every PhiColour / PhiNormal of test_atrous, clean and poisoned) and TAA, case by case (twin_case)."""
    fma_or_skip(ref)
    W, H = size
    O, OF, RF = rc.OracleSide(ref), rc.OracleSide(ref, "fma"), rc.ReferenceSide(ref, fma=True)
    worst = (0.0, 0.0)
    for poison in (False, True):
        _, f1 = rc.frame_pair(W, H, poison=poison)
        src, _, hist, marker = rc.spatial_inputs(W, H, poison=poison)
        for (pc, pn), it in itertools.product(PHI, (0, 1)):
            o, of, rf = (s.atrous(W, H, src, marker, gbuf(f1), hist, step=step, phi_colour=pc, phi_normal=pn, iteration=it) for s in (O, OF, RF))
            what = f"fma twin a-trous {W}x{H} step {step} iteration {it} phi {pc}/{pn} poison {poison}"
            worst = max(worst, twin_case(o[0], of[0], rf[0], what))
            if it:
                exact(rf[1], marker, what + ": no feedback")
            if it == 0:
                twin_case(o[1], of[1], rf[1], what + ": feedback")
        if step == 1:
            filt, th = rc.taa_inputs(W, H, poison=poison)
            r = twin_case(O.taa(W, H, filt, th), OF.taa(W, H, filt, th), RF.taa(W, H, filt, th), f"fma twin TAA {W}x{H} poison {poison}")
            print(f"TAA {W}x{H} poison {poison}: fma twin residual {r[0]:.3e}, envelope {r[1]:.3e}")
    print(f"a-trous {W}x{H} step {step}: largest fma twin residual {worst[0]:.3e}, that case's envelope {worst[1]:.3e}")


@pytest.mark.parametrize("size", rc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fma_twin_sequence(ref, size):
    """The twin's six frames: history exact, every other state plane of every frame case by case (twin_case)."""
    fma_or_skip(ref)
    W, H = size
    o, of, rf = rc.oracle_sequence(ref, W, H), rc.oracle_sequence(ref, W, H, "fma"), rc.reference_sequence(ref, W, H, fma=True)
    for k, (a, b, c) in enumerate(zip(o, of, rf)):
        assert np.array_equal(b["hist"], c["hist"]), f"frame {k}: history"
        for plane in ("colour", "mom", "out"):
            r = twin_case(a[plane], b[plane], c[plane], f"fma twin sequence {W}x{H} frame {k}: {plane}")
            print(f"sequence {W}x{H} frame {k} {plane}: fma twin residual {r[0]:.3e}, envelope {r[1]:.3e}")


# ------------------------------------------------------------------------------------------------------------------------------ fixtures
def _load(name):
    z = np.load(os.path.join(GOLD, name))
    params = {k[len("param_"):]: z[k] for k in z.files if k.startswith("param_")}
    return params, {k: z[k] for k in z.files if not k.startswith("param_")}


def test_recorded_parameters_are_the_cases_parameters():
    for name in ("ref_stages_64x48.npz", "ref_sequence_64x48.npz"):
        params, _ = _load(name)
        assert sorted(params) == sorted(rc.FIXTURE_PARAMS)
        for k, v in rc.FIXTURE_PARAMS.items():
            assert np.array_equal(params[k], np.asarray(v)), (name, k)
        assert os.path.getsize(os.path.join(GOLD, name)) <= 332017             # no larger than the largest fixture before them (atrous_96x64.npz)


def test_oracle_reproduces_recorded_reference_stages(oracle):
    """Always on: the oracle against what the reference build computed (tests/golden/ref_stages_64x48.npz), bit for bit, from regenerated inputs."""
    params, want = _load("ref_stages_64x48.npz")
    got = rc.fixture_stage_outputs(rc.OracleSide(oracle), params)
    assert sorted(got) == sorted(want) and len(want) == 11
    for k in want:
        exact(got[k], want[k], f"recorded reference {k}")
    assert np.isnan(want["moments_poison"].astype(np.float32)).any() and np.isnan(want["atrous_step1_it0_poison"].astype(np.float32)).any()


def test_oracle_reproduces_recorded_reference_sequence(oracle):
    params, want = _load("ref_sequence_64x48.npz")
    W, H = int(params["W"]), int(params["H"])
    got = rc.fixture_sequence_outputs(rc.oracle_sequence(oracle, W, H, frames=int(params["sequence_frames"]), steps=int(params["sequence_steps"]),
                                                         mv=tuple(float(v) for v in params["mv"])))
    for k in want:
        exact(got[k], want[k], f"recorded reference sequence {k}")


def test_recorded_fixtures_are_current(ref):
    """With oracle/_ref present: the fixture files hold exactly what the reference build computes now."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(GOLD, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    for name, arrays in mg.reference_fixtures().items():
        z = np.load(os.path.join(GOLD, name))
        assert sorted(z.files) == sorted(arrays), name
        for k, v in arrays.items():
            v = np.asarray(v)
            assert z[k].dtype == v.dtype and z[k].shape == v.shape and np.array_equal(rc.bits(z[k]) if v.dtype.kind == "f" and v.dtype.itemsize in (2, 4) else z[k],
                                                                                     rc.bits(v) if v.dtype.kind == "f" and v.dtype.itemsize in (2, 4) else v), (name, k)
