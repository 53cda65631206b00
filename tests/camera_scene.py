"""A camera moving through a small analytic world: per-pixel motion for the filter's tests (test infrastructure, CPU, NumPy).

svgf_amd/synth.py feeds every other test with ONE motion vector for the whole frame (a constant pan).  A host of the reference renders
GBuffer.frag motion instead: camera rotation, dolly and parallax make the vector differ from texel to texel, an object that moves by itself
gets motion the matrices do not explain, and what it uncovers is young.  This module ray-casts such frames in float64 and stores them in
float32 as the linear attribute planes the G-buffer adapter (svgf_pack_gbuffer) reads; the G-buffer itself comes from the oracle's adapter
(oracle.pack_gbuffer), to which the device adapter is held bit for bit.

  position  float32[H, W, 4]  (x, y, z, 1) of the surface point; 0 on sky
  normal    float32[H, W, 4]  (nx, ny, nz, matID = instance + 10); all 0 on sky (GBuffer.frag's cleared texels)
  bary      float32[H, W, 4]  (b0, b1, b2, instanceID): what the mesh test reads as uv[3]
  vp, prev_vp                 16 float32, column-major (glm), of this frame and the previous one; eye: float32[3]

Pixel (x, y) is the NDC point ((x + 0.5) / W * 2 - 1, (y + 0.5) / H * 2 - 1): row 0 is the bottom of the image, as in GL's window
coordinates, so that motion = (prev NDC - cur NDC) * (W/2, H/2) is the pixel offset to where the point was seen (GBuffer.frag:67-71).

Camera paths (PATHS): orbit (rotation + parallax), dolly (radial motion), roll (rotation about the view axis), pan (fast diagonal, with a
vertical component), whip (a slow orbit with one sudden 20-degree turn: the share of young pixels jumps above the frame driver's adaptive
threshold and falls back under the lower one).  Every path has the moving sphere.  Radiance: a pattern anchored in the world times seeded
1-spp noise (synth._noise_rows' model: a path finds the light with p = 1/4 and carries 4x the radiance)."""
from __future__ import annotations

import functools

import numpy as np

from svgf_amd import synth

PATHS = ("orbit", "dolly", "roll", "pan", "whip")
SEED = 0x43414D5343454E45          # "CAMSCENE"
SKY = 0
MOVER = 7                           # the instance that moves between frames
FOVY = np.radians(55.0)
ZNEAR, ZFAR = 0.1, 100.0
GROUND_REACH = 60.0                 # the ground ends there (beyond: sky)

# instance -> albedo
_ALBEDO = np.array([[0.25, 0.45, 0.80], [0.45, 0.50, 0.40], [0.80, 0.25, 0.20], [0.20, 0.55, 0.85], [0.85, 0.80, 0.75],
                    [0.90, 0.85, 0.30], [0.30, 0.75, 0.35], [0.85, 0.35, 0.80]], np.float64)
_BOXES = [(2, (-2.6, 0.0, -1.6), (-1.0, 1.8, 0.0)),       # (instance, min corner, max corner), axis-aligned
          (3, (1.2, 0.0, -3.6), (2.7, 1.1, -2.2)),
          (4, (0.45, 0.0, 1.15), (0.62, 2.6, 1.32))]      # a thin pole: thin geometry under motion
_SPHERES = [(5, (0.3, 0.9, -0.9), 0.9), (6, (-0.7, 0.5, 2.1), 0.5)]
_LIGHT = np.array([0.4, 0.8, 0.45]) / np.linalg.norm([0.4, 0.8, 0.45])


def mover_centre(k):
    return np.array([-1.9 + 0.14 * k, 0.55 + 0.03 * np.sin(k), 1.0 - 0.05 * k])


def look_at(eye, target, up=(0.0, 1.0, 0.0)):
    e, t, u = (np.asarray(v, np.float64) for v in (eye, target, up))
    f = t - e
    f /= np.linalg.norm(f)
    s = np.cross(f, u)
    s /= np.linalg.norm(s)
    uu = np.cross(s, f)
    m = np.eye(4)
    m[0, :3], m[1, :3], m[2, :3] = s, uu, -f
    m[:3, 3] = -m[:3, :3] @ e
    return m


def perspective(fovy, aspect, zn=ZNEAR, zf=ZFAR):
    t = 1.0 / np.tan(fovy / 2)
    m = np.zeros((4, 4))
    m[0, 0], m[1, 1] = t / aspect, t
    m[2, 2], m[2, 3], m[3, 2] = (zf + zn) / (zn - zf), 2 * zf * zn / (zn - zf), -1.0
    return m


def colmajor(m):
    return np.ascontiguousarray(m.T, np.float32).ravel()


def camera(path, k):
    """(eye, target, up) of frame k of a path."""
    tgt = np.array([0.0, 0.7, 0.0])
    up = np.array([0.0, 1.0, 0.0])

    def orbit_at(a, r=7.5, h=2.2):
        return np.array([r * np.sin(a), h, r * np.cos(a)])
    if path == "static":
        return orbit_at(0.35), tgt, up
    if path == "orbit":
        return orbit_at(0.35 + 0.02 * k, h=2.2 + 0.03 * k), tgt, up
    if path == "dolly":
        e0 = orbit_at(0.2, r=8.5, h=2.6)
        d = (tgt - e0) / np.linalg.norm(tgt - e0)
        return e0 + d * (0.2 * k) + np.array([0.0, 0.02 * k, 0.0]), tgt, up
    if path == "roll":
        e = orbit_at(-0.3)
        f = (tgt - e) / np.linalg.norm(tgt - e)
        a = 0.025 * k
        s = np.cross(f, up)
        s /= np.linalg.norm(s)
        u0 = np.cross(s, f)
        return e, tgt, np.cos(a) * u0 + np.sin(a) * s
    if path == "pan":
        d = np.array([0.2, 0.09, -0.04]) * k
        return orbit_at(0.1) + d - np.array([0.8, 0.3, 0.0]), tgt + d - np.array([0.8, 0.3, 0.0]), up
    if path == "whip":
        a = 0.45 + 0.012 * k + (0.35 if k >= WHIP_FRAME else 0.0)
        return orbit_at(a, r=7.0), tgt, up
    raise ValueError(path)


WHIP_FRAME = 5


def view_proj(path, k, W, H):
    eye, tgt, up = camera(path, k)
    return perspective(FOVY, W / H) @ look_at(eye, tgt, up), eye


def raycast(path, k, W, H, px, py):
    """Rays through the continuous pixel coordinates (px, py) (pixel centres at +0.5) of frame k -> (instance int32, t, point, normal)."""
    eye, tgt, up = camera(path, k)
    f = (tgt - eye) / np.linalg.norm(tgt - eye)
    s = np.cross(f, up)
    s /= np.linalg.norm(s)
    u = np.cross(s, f)
    th = np.tan(FOVY / 2)
    a = ((px / W * 2.0 - 1.0) * (th * W / H)).ravel()
    b = ((py / H * 2.0 - 1.0) * th).ravel()
    d = [f[i] + a * s[i] + b * u[i] for i in range(3)]
    inv_len = 1.0 / np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    for i in range(3):
        d[i] *= inv_len
    n_rays = a.size
    best = np.full(n_rays, np.inf)
    inst = np.zeros(n_rays, np.int32)
    nrm = np.zeros((n_rays, 3))
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = [1.0 / d[i] for i in range(3)]
        # ground y = 0
        t = -eye[1] * inv[1]
        hit = (t > 0) & (t < GROUND_REACH)
        inst[hit], best[hit], nrm[hit] = 1, t[hit], (0.0, 1.0, 0.0)
        for iid, lo, hi in _BOXES:
            tmin, tn, tf = [], None, None
            for i in range(3):
                t1, t2 = (lo[i] - eye[i]) * inv[i], (hi[i] - eye[i]) * inv[i]
                tmin.append(np.minimum(t1, t2))
                tmax = np.maximum(t1, t2)
                tn = tmin[i] if tn is None else np.maximum(tn, tmin[i])
                tf = tmax if tf is None else np.minimum(tf, tmax)
            hit = (tn <= tf) & (tn > 0) & (tn < best)
            idx = np.nonzero(hit)[0]
            n = np.zeros((idx.size, 3))
            ax = np.where(tmin[0][idx] == tn[idx], 0, np.where(tmin[1][idx] == tn[idx], 1, 2))
            n[np.arange(idx.size), ax] = -np.sign(np.where(ax == 0, d[0][idx], np.where(ax == 1, d[1][idx], d[2][idx])))
            inst[idx], best[idx], nrm[idx] = iid, tn[idx], n
        for iid, c, r in _SPHERES + [(MOVER, mover_centre(k), 0.45)]:
            oc = eye - np.asarray(c)
            bq = d[0] * oc[0] + d[1] * oc[1] + d[2] * oc[2]
            disc = bq * bq - (oc @ oc - r * r)
            t = -bq - np.sqrt(disc)
            idx = np.nonzero((disc > 0) & (t > 0) & (t < best))[0]
            inst[idx], best[idx] = iid, t[idx]
            nrm[idx] = (eye[None, :] + t[idx, None] * np.stack([d[i][idx] for i in range(3)], -1) - np.asarray(c)[None, :]) / r
    p = eye[None, :] + best[:, None] * np.stack(d, -1)
    p[inst == SKY] = 0.0
    return inst.reshape(px.shape), best.reshape(px.shape), p.reshape(px.shape + (3,)), nrm.reshape(px.shape + (3,))


_CHUNK = 256


def _attributes(path, k, W, H):
    """The adapter's input planes and the noise-free radiance of frame k."""
    pos = np.zeros((H, W, 4), np.float32)
    nrm = np.zeros((H, W, 4), np.float32)
    bary = np.zeros((H, W, 4), np.float32)
    base = np.empty((H, W, 3), np.float32)
    region = np.empty((H, W), np.int32)
    xs = np.arange(W, dtype=np.float64) + 0.5
    for a in range(0, H, _CHUNK):
        b = min(a + _CHUNK, H)
        py, px = np.meshgrid(np.arange(a, b, dtype=np.float64) + 0.5, xs, indexing="ij")
        inst, _, p, n = raycast(path, k, W, H, px, py)
        cov = inst != SKY
        # the point in the object's own frame: the mover's pattern moves with it
        q = p - np.where((inst == MOVER)[..., None], mover_centre(k)[None, None, :], 0.0)
        pos[a:b, ..., :3] = p
        pos[a:b, ..., 3] = np.where(cov, 1.0, 0.0)
        nrm[a:b, ..., :3] = n
        nrm[a:b, ..., 3] = np.where(cov, inst + 10, 0)
        b0 = np.abs(np.sin(3.1 * q[..., 0] + 1.7 * q[..., 2]))
        b1 = np.abs(np.sin(2.3 * q[..., 1] - 2.9 * q[..., 2])) * (1.0 - b0)
        bary[a:b] = np.stack([b0, b1, 1.0 - b0 - b1, inst.astype(np.float64)], -1) * cov[..., None]
        shade = 0.35 + 0.65 * np.clip(n @ _LIGHT, 0.0, 1.0)
        tex = 0.75 + 0.25 * np.sin(5.0 * q[..., 0]) * np.sin(5.0 * q[..., 2] + 1.0) * np.cos(3.0 * q[..., 1])
        col = _ALBEDO[inst] * (shade * tex)[..., None] * 0.7 + 0.04
        col[~cov] = _ALBEDO[SKY]
        base[a:b] = col
        region[a:b] = inst
    return pos, nrm, bary, base, region


def radiance(base, frame, seed=SEED):
    """1-spp radiance {r, g, b, 1}: synth._noise_rows' model on this scene's noise-free colour."""
    H, W = base.shape[:2]
    hit = synth.uniform01(seed, frame + 1, np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), 0) < np.float32(0.25)
    out = np.empty((H, W, 4), np.float32)
    out[..., :3] = np.clip(np.where(hit[..., None], base * np.float32(4.0), np.float32(0.0)), 0.0, 1.0)
    out[..., 3] = 1.0
    return out


def make_frame(path, k, W, H, seed=SEED, static=False):
    """Frame k of a path: dict(position, normal_in, bary, vp, prev_vp, eye, motion, normal, uv, radiance, region, base).
    static: prev_vp = vp (the camera did not move since the previous frame)."""
    from oracle import oracle as orc
    pos, nrm, bary, base, region = _attributes(path, k, W, H)
    vp, eye = view_proj(path, k, W, H)
    pvp = vp if static or k == 0 else view_proj(path, k - 1, W, H)[0]
    fr = dict(position=pos, normal_in=nrm, bary=bary, vp=colmajor(vp), prev_vp=colmajor(pvp), eye=eye.astype(np.float32), region=region, base=base)
    fr["motion"], fr["normal"], fr["uv"] = orc.pack_gbuffer(pos, nrm, bary, fr["vp"], fr["prev_vp"], fr["eye"])
    fr["radiance"] = radiance(base, k, seed)
    return fr


@functools.lru_cache(maxsize=16)
def sequence(path, W, H, N, seed=SEED):
    """N frames of a path (cached: a sequence is made once per process)."""
    return tuple(make_frame(path, k, W, H, seed) for k in range(N))


def prev_pixel(path, k, W, H, point):
    """Continuous pixel coordinates of world points in frame k - 1's camera (float64): where the point was seen."""
    vp, _ = view_proj(path, k - 1, W, H)
    ph = np.concatenate([point, np.ones(point.shape[:-1] + (1,))], -1) @ vp.T
    return (ph[..., 0] / ph[..., 3] + 1.0) * 0.5 * W, (ph[..., 1] / ph[..., 3] + 1.0) * 0.5 * H


def rzi(v):
    """cvt.rzi.s32.f32 (Filter.cuh:232): toward zero, saturating, NaN -> 0."""
    v = np.nan_to_num(np.asarray(v, np.float64), nan=0.0)
    return np.clip(np.trunc(v), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)


def reprojection(frame):
    """(qx, qy, inside the frame) of every pixel: where the temporal stage reads the previous frame (Filter.cuh:232-235)."""
    H, W = frame["motion"].shape[:2]
    Y, X = np.mgrid[0:H, 0:W]
    qx, qy = X + rzi(frame["motion"][..., 0]), Y + rzi(frame["motion"][..., 1])
    return qx, qy, (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)


# ------------------------------------------------------------------ the frame driver's sample of young pixels (svgf_kernels.hip:temporal_kernel)
def listed_young(hist, normal_bits, phi_normal=128.0):
    """The pixels the temporal launch lists for the young-pixel launch: history < 4, except a zero normal's when PhiNormal > 0."""
    zero = ((normal_bits[..., 0] & 0x7FFF) | (normal_bits[..., 1] & 0x7FFF) | (normal_bits[..., 2] & 0x7FFF)) == 0
    return (hist < 4) & ~(zero & (phi_normal > 0))


def wave_masks(listed):
    """-> (popcount, all 64 lanes set) per (row, 64-column wave); lanes beyond W are 0."""
    H, W = listed.shape
    nw = (W + 63) // 64
    pad = np.zeros((H, nw * 64), bool)
    pad[:, :W] = listed
    cnt = pad.reshape(H, nw, 64).sum(-1)
    return cnt, cnt == 64


def young_sample(listed, y0=0):
    """The sample one temporal launch adds up (one wave in 64, hashed over wave and row) -> (young pixels, waves that hold some but not 64),
    as svgf_adaptive_moments_sample reports them (x 64, saturated)."""
    cnt, full = wave_masks(listed)
    H, nw = cnt.shape
    bx, y = np.meshgrid(np.arange(nw, dtype=np.int64), np.arange(y0, y0 + H, dtype=np.int64))
    pick = (((bx * 29 + y * 13) & 0xFFFFFFFF) & 63) == 0
    pick &= cnt > 0
    px, wv = int(cnt[pick].sum()), int((pick & ~full).sum())
    return min(64 * px, 0xFFFFFFFF), min(64 * wv, 0xFFFFFFFF)


def young_append_cap(rows, W):
    waves = rows * ((W + 63) // 64)
    cap = waves // 4 if waves // 4 > 1024 else 1024
    return cap // 8 * 8


def adaptive_states(samples, W, H, cold=3):
    """The frame driver's choice (svgf_api.hip:choose_moments_kernel) frame by frame when every frame is synchronised before the next:
    frame j reads the sample of frame j - 2 (published by frame j - 1's temporal launch).  samples[j]: young_sample of frame j (cold frames
    add nothing).  -> list of dense_moments after each frame's choice."""
    dense, out = False, []
    cap = young_append_cap(H, W)
    for j in range(len(samples)):
        if j >= cold:
            s = samples[j - 2] if j >= 2 and j - 2 >= cold else (0, 0)
            est, appends = s[0] / (W * H), s[1]
            if est > 0.08 or appends > cap:
                dense = True
            elif est < 0.05 and appends < cap // 4 * 3:
                dense = False
        out.append(dense)
    return out
