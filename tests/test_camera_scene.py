"""CPU self-checks of tests/camera_scene.py: the scene's motion must be right (else every pixel is rejected and the GPU tests of
tests/test_gpu_camera_motion.py exercise only cold frames) and must hold what those tests claim to cover."""
import numpy as np
import pytest

from oracle import svgf_numpy as snp
from tests import camera_scene as cs
from tests.helpers import gbuf

W, H, N = 517, 333, 12


def _hist_sequence(oracle, fr):
    """The oracle's temporal stage over a sequence -> the history plane of every frame."""
    hp = np.zeros((H, W), np.uint8)
    z4, z2 = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 2), np.float32)
    out = []
    for k in range(len(fr)):
        hc = np.zeros_like(hp)
        oracle.temporal(W, H, "f32", z4, fr[k]["radiance"], z4.copy(), gbuf(fr[k]), gbuf(fr[max(k - 1, 0)]), hp, hc, z2.copy(), z2,
                        depth_threshold=0.8, normal_threshold=0.9, history_base=24, mesh_id_test=1)
        out.append(hc)
        hp = hc
    return out


@pytest.mark.parametrize("path", cs.PATHS)
def test_motion_lands_where_the_point_was_seen(path):
    """On >= 99 % of the texels that see a static point visible in the previous frame too, p + rzi(mv) is within 1 px (each axis) of the
    pixel of the previous frame that saw it — the adapter's NDC and sign conventions and the scene's pixel-to-ray mapping agree."""
    fr = cs.sequence(path, W, H, N)
    worst = 1.0
    for k in (1, 4, 7):
        f = fr[k]
        cov = (f["region"] != cs.SKY) & (f["region"] != cs.MOVER)
        px, py = cs.prev_pixel(path, k, W, H, f["position"][..., :3].astype(np.float64))
        inside = cov & (px >= 0) & (px < W) & (py >= 0) & (py < H)
        # visible in frame k - 1: the ray through (px, py) of that frame hits the same point
        _, _, seen, _ = cs.raycast(path, k - 1, W, H, np.where(inside, px, 0.5), np.where(inside, py, 0.5))
        vis = inside & (np.linalg.norm(seen - f["position"][..., :3], axis=-1) < 1e-3 * (1 + np.linalg.norm(f["position"][..., :3], axis=-1)))
        assert vis.mean() > 0.5, f"{path} frame {k}: only {vis.mean():.2f} of the frame seen twice"
        qx, qy, _ = cs.reprojection(f)
        near = (np.abs(qx - np.floor(px)) <= 1) & (np.abs(qy - np.floor(py)) <= 1)
        worst = min(worst, float(near[vis].mean()))
    assert worst >= 0.99, f"{path}: motion lands within 1 px on {worst:.4f} of the texels seen twice"


def test_a_static_camera_gives_zero_motion(oracle):
    f = cs.make_frame("static", 3, W, H, static=True)
    cov = f["region"] != cs.SKY
    assert cov.mean() > 0.5 and (~cov).any()
    assert np.all(f["motion"][cov][:, :2] == 0) and np.all(f["motion"][~cov] == 0)


@pytest.mark.parametrize("path", cs.PATHS)
def test_the_two_adapters_agree_on_the_scene(path):
    """The C++ oracle's adapter (which made the planes) against its NumPy twin, once per path."""
    f = cs.sequence(path, W, H, N)[6]
    for a, b in zip((f["motion"], f["normal"], f["uv"]), snp.pack_gbuffer(f["position"], f["normal_in"], f["bary"], f["vp"], f["prev_vp"], f["eye"])):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("path", cs.PATHS)
def test_every_path_has_steady_and_cold_pixels_and_varied_motion(oracle, path):
    """With the oracle's temporal stage, every frame after the first accepts between 30 % and 99.9 % of the covered texels; each path has more
    than 20 distinct (rzi(mv.x), rzi(mv.y)); young pixels (listed ones: history < 4, not zero-normal) sit in >= 10 % of the 64-pixel waves
    of every frame from the fourth on, and most such waves are only partly young."""
    fr = cs.sequence(path, W, H, N)
    hists = _hist_sequence(oracle, fr)
    distinct = set()
    for k in range(1, N):
        cov = fr[k]["region"] != cs.SKY
        acc = float((hists[k] > 1)[cov].mean())
        assert 0.3 <= acc <= 0.999, f"{path} frame {k}: {acc:.3f} of the covered texels accepted"
        mv = fr[k]["motion"]
        distinct |= set(zip(cs.rzi(mv[..., 0][cov]).tolist(), cs.rzi(mv[..., 1][cov]).tolist()))
        if k >= 3:
            cnt, full = cs.wave_masks(cs.listed_young(hists[k], fr[k]["normal"]))
            some = cnt > 0
            assert some.mean() >= 0.1, f"{path} frame {k}: young pixels in {some.mean():.3f} of the waves"
            assert (some & ~full).sum() > 0.5 * some.sum(), f"{path} frame {k}: most young waves are all young"
    assert len(distinct) > 20, f"{path}: {len(distinct)} distinct motion vectors"


def test_the_whip_crosses_the_adaptive_thresholds_both_ways(oracle):
    """The frame driver's sample (restated: one wave in 64) goes above 8 % at the turn and back below 5 %: the dense moments kernel is chosen
    and left again within the twelve frames."""
    fr = cs.sequence("whip", W, H, N)
    hists = _hist_sequence(oracle, fr)
    samples = [cs.young_sample(cs.listed_young(h, f["normal"])) if k >= 3 else (0, 0) for k, (h, f) in enumerate(zip(hists, fr))]
    est = [s[0] / (W * H) for s in samples]
    assert max(est[3:cs.WHIP_FRAME]) < 0.05 and est[cs.WHIP_FRAME] > 0.08 and est[-1] < 0.05, est
    states = cs.adaptive_states(samples, W, H)
    on = states.index(True)
    assert not all(states[on:]), states


def test_4k_frames_are_quick():
    import time
    t = time.perf_counter()
    f = cs.make_frame("orbit", 2, 3840, 2160)
    assert f["motion"].shape == (2160, 3840, 4)
    assert time.perf_counter() - t < 15.0
