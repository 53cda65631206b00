"""The size-dependent launch geometry of the streaming kernels, restated on the host (test infrastructure; no GPU).

The launchers cut their work by the chip's CU count (svgf_device.h:num_cus): how long a band of rows one workgroup streams down is, how many
bands a frame has, how the tiles are grouped per XCD.  A test that claims to cover the long bands of a 4K or 8K frame asks this module what the
launch it checks really looks like, and asserts it (tests/test_gpu_fullsize_parity.py); tests/test_launch_geometry.py pins it on the numbers
the documents quote.

The named constants are read out of the headers, so that a change there shows here.  The literals of the launchers' formulas are restated by
hand; `_FORMS` holds the C++ text each restatement follows, and every call checks that the headers still hold it (GeometryDrift otherwise)."""
from __future__ import annotations

import functools
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "svgf_amd", "csrc")
HEADERS = ("svgf_device.h", "svgf_atrous_lds.h", "svgf_moments_lds.h", "svgf_atrous_fused.h", "svgf_kernels.h", "svgf_kernels.hip")
LDS_PER_CU = 160 * 1024                      # the launchers' (160 * 1024) / lds


class GeometryDrift(AssertionError):
    """The C++ no longer holds a formula this module restates: the restatement must be updated with it."""


# (file, exact C++ text) of every formula restated below with its literals
_FORMS = [
    ("svgf_atrous_lds.h", "static constexpr size_t bytes = (size_t)kRing * WL * kRecBytes + (kRing * 8 + 14) * sizeof(uint32_t);"),
    ("svgf_atrous_lds.h", "static constexpr int WL = TX + 4 * S;"),
    ("svgf_atrous_lds.h", "const int per_cu_lds = (int)((160 * 1024) / lds), per_cu_waves = atrous_waves(S) * 4 / (TX * kRS / 64);"),
    ("svgf_atrous_lds.h", "nbands = per_cu * num_cus() * kAtrousOversubscribe / (xtiles * S);"),
    ("svgf_atrous_lds.h", "band = (njmax + nbands - 1) / nbands;"),
    ("svgf_atrous_lds.h", "if (band < kAtrousMinBand) band = kAtrousMinBand;"),
    ("svgf_atrous_lds.h", "band = (band + kRS - 1) / kRS * kRS;"),
    ("svgf_atrous_lds.h", "xcd_grid(last_tiles, S <= 2 ? 16 : (S == 16 ? 2 : 1), rp.xgroup)"),
    ("svgf_atrous_lds.h", "const int nt = rp.ye[r] > rp.yb[r] ? xtiles * rp.nbands[r] * S : 0;"),
    ("svgf_atrous_lds.h", "launch_atrous_lds_tx<ST, S, kTX>(g, a, s, r)"),
    ("svgf_device.h", "xgroup = (ntiles + kXcds * xm - 1) / (kXcds * xm);"),
    ("svgf_device.h", "return dim3((unsigned)((ngroups + kXcds - 1) / kXcds) * kXcds * xgroup);"),
    ("svgf_moments_lds.h", "constexpr size_t lds = (size_t)kMRing * WL * kMRecBytes + (kMRing * 4 + 1 + 2) * sizeof(uint32_t);"),
    ("svgf_moments_lds.h", "constexpr int WL = kMTX + 2 * kMR;"),
    ("svgf_moments_lds.h", "int nbands = kMRounds * per_cu * num_cus() / xtiles;"),
    ("svgf_moments_lds.h", "if (band < 8) band = 8;"),
    ("svgf_atrous_fused.h", "int nbands = 2 * num_cus() * 2 / xtiles;"),
    ("svgf_atrous_fused.h", "if (band < 32) band = 32;"),
    ("svgf_atrous_fused.h", "band = (band + 1) / 2 * 2;"),
    ("svgf_atrous_fused.h", "const dim3 grid = xcd_grid(xtiles * nbands, 16, xgroup);"),
    ("svgf_kernels.hip", "int scan = (nsegs + 255) / 256;"),
    ("svgf_kernels.hip", "if (scan > 4 * num_cus()) scan = 4 * num_cus();"),
    ("svgf_kernels.hip", "const int walk = std::min(4 * num_cus(), std::max(1, nsegs / 16));"),
    ("svgf_kernels.hip", "scan *= kScanSplit;"),
    ("svgf_kernels.hip", "const int nsegs = (g.ye - g.yb) * ((g.W + kBX - 1) / kBX);"),
    ("svgf_kernels.h", "const long long waves = (long long)rows * ((W + 63) / 64);"),
    ("svgf_kernels.h", "const long long cap = waves / 4 > 1024 ? waves / 4 : 1024;"),
    ("svgf_kernels.h", "return (unsigned)(cap / kYoungShards * kYoungShards);"),
]
_ATROUS_WAVES = re.compile(r"constexpr int atrous_waves\(int S\) \{ return S <= 8 \? (\d+) : S == 16 \? (\d+) : S == 32 \? (\d+) : (\d+); \}")
_CONST = re.compile(r"constexpr (?:int|unsigned|size_t) (k[A-Za-z0-9]+ = [^;]+);")
_NEEDED = ("kTX", "kRS", "kRing", "kRecBytes", "kXcds", "kAtrousOversubscribe", "kAtrousMinBand", "kMR", "kMRing", "kMTX", "kMRounds",
           "kMRecBytes", "kFT0", "kFReach1", "kFT1", "kBX", "kScanSplit", "kYoungShards")


@functools.lru_cache(maxsize=None)
def constants() -> dict:
    """The named constants the formulas use, read out of the headers (each `constexpr int kName = expr;` evaluated over the ones before it),
    plus `atrous_waves` as {step: waves}.  Raises GeometryDrift if a formula of _FORMS or a constant is gone."""
    text = {h: open(os.path.join(CSRC, h)).read() for h in HEADERS}
    squash = {h: " ".join(t.split()) for h, t in text.items()}
    for h, form in _FORMS:
        if form not in squash[h]:
            raise GeometryDrift(f"{h} no longer holds `{form}`: tests/launch_geometry.py restates it")
    c = {}
    for h in HEADERS:
        for decl in _CONST.findall(text[h]):
            for part in re.sub(r"//.*", "", decl).rstrip(";").split(","):      # (constexpr int kBX = 64, kBY = 4;)
                name, _, expr = part.partition("=")
                name, expr = name.strip(), expr.strip()
                if not re.fullmatch(r"[\sA-Za-z0-9_+\-*/()]+", expr):
                    continue
                try:
                    c[name] = int(eval(expr.replace("/", "//"), {"__builtins__": {}}, dict(c)))   # noqa: S307  (integers and earlier names only)
                except (NameError, SyntaxError, TypeError):
                    continue
    missing = [n for n in _NEEDED if n not in c]
    if missing:
        raise GeometryDrift(f"constants not found in the headers: {missing}")
    m = _ATROUS_WAVES.search(text["svgf_atrous_lds.h"])
    if not m:
        raise GeometryDrift("svgf_atrous_lds.h: atrous_waves(S) changed form")
    w = [int(v) for v in m.groups()]
    c["atrous_waves"] = {1: w[0], 2: w[0], 4: w[0], 8: w[0], 16: w[1], 32: w[2], 64: w[3]}
    return c


def xcd_grid(ntiles: int, xm: int) -> tuple[int, int]:
    """svgf_device.h:xcd_grid — -> (workgroups launched, xgroup).  Workgroups beyond ntiles are padding (they return at once)."""
    k = constants()["kXcds"]
    xgroup = max(1, (ntiles + k * xm - 1) // (k * xm))
    ngroups = (ntiles + xgroup - 1) // xgroup
    return (ngroups + k - 1) // k * k * xgroup, xgroup


def atrous_lds_bytes(S: int) -> int:
    """svgf_atrous_lds.h:AtrousLds<S, kTX>::bytes (:39,47)."""
    c = constants()
    WL = c["kTX"] + 4 * S
    return c["kRing"] * WL * c["kRecBytes"] + (c["kRing"] * 8 + 14) * 4


def atrous_lds(W: int, rows: int, S: int, num_cus: int) -> dict:
    """One launch of atrous_lds_kernel over `rows` rows of a W-wide frame at step S (a whole-frame stage call: rows = H) —
    svgf_atrous_lds.h:cut_bands (:354-364) and launch_atrous_lds_tx (:371, 383, 393).
    -> band (decimated rows per band), nbands, xtiles, tiles, blocks, xgroup, padding (blocks - tiles), last_band (rows of the last band of
       row residue 0; equal to `band` when the cut is even), per_cu, lds."""
    c = constants()
    TX, RS = c["kTX"], c["kRS"]
    lds = atrous_lds_bytes(S)
    per_cu = min(LDS_PER_CU // lds, c["atrous_waves"][S] * 4 // (TX * RS // 64))
    xtiles = (W + TX - 1) // TX
    njmax = (rows + S - 1) // S
    nbands = max(1, per_cu * num_cus * c["kAtrousOversubscribe"] // (xtiles * S))
    band = (njmax + nbands - 1) // nbands
    band = max(band, c["kAtrousMinBand"])
    band = (band + RS - 1) // RS * RS
    nbands = (njmax + band - 1) // band
    tiles = xtiles * nbands * S
    xm = 16 if S <= 2 else (2 if S == 16 else 1)
    blocks, xgroup = xcd_grid(tiles, xm)
    return dict(band=band, nbands=nbands, xtiles=xtiles, tiles=tiles, blocks=blocks, xgroup=xgroup, padding=blocks - tiles,
                last_band=njmax - (nbands - 1) * band, per_cu=per_cu, lds=lds)


def moments_lds(W: int, rows: int, num_cus: int) -> dict:
    """One launch of moments_lds_kernel — svgf_moments_lds.h:launch_moments_lds (:278-290).  -> band, nbands, xtiles, per_cu, lds."""
    c = constants()
    WL = c["kMTX"] + 2 * c["kMR"]
    lds = c["kMRing"] * WL * c["kMRecBytes"] + (c["kMRing"] * 4 + 1 + 2) * 4
    per_cu = LDS_PER_CU // lds
    xtiles = (W + c["kMTX"] - 1) // c["kMTX"]
    nbands = max(1, c["kMRounds"] * per_cu * num_cus // xtiles)
    band = max((rows + nbands - 1) // nbands, 8)
    band = (band + c["kRS"] - 1) // c["kRS"] * c["kRS"]
    nbands = (rows + band - 1) // band
    return dict(band=band, nbands=nbands, xtiles=xtiles, per_cu=per_cu, lds=lds, last_band=rows - (nbands - 1) * band)


def atrous_fused12(W: int, rows: int, num_cus: int) -> dict:
    """One launch of atrous_fused12_kernel (iterations 0 + 1) over iteration 1's rows — svgf_atrous_fused.h:launch_atrous_fused12 (:297-307).
    -> band, nbands, xtiles, tiles, blocks, xgroup, padding, last_band."""
    c = constants()
    xtiles = (W + c["kFT1"] - 1) // c["kFT1"]
    nbands = max(1, 2 * num_cus * 2 // xtiles)
    band = max((rows + nbands - 1) // nbands, 32)
    band = (band + 1) // 2 * 2
    nbands = (rows + band - 1) // band
    tiles = xtiles * nbands
    blocks, xgroup = xcd_grid(tiles, 16)
    return dict(band=band, nbands=nbands, xtiles=xtiles, tiles=tiles, blocks=blocks, xgroup=xgroup, padding=blocks - tiles,
                last_band=rows - (nbands - 1) * band)


def young_append_cap(rows: int, W: int) -> int:
    """svgf_kernels.h:young_append_cap (:23-27): appends the young-pixel list takes per frame, over all shards."""
    waves = rows * ((W + 63) // 64)
    cap = waves // 4 if waves // 4 > 1024 else 1024
    k = constants()["kYoungShards"]
    return cap // k * k


def young_launch(W: int, rows: int, num_cus: int) -> dict:
    """The young-pixel launch of the moments stage (moments_young_kernel) — svgf_kernels.hip:launch_moments (:927-936).
    -> nsegs (64-column segments), scan (mask-scanning workgroups, kScanSplit per slot), walk (list-walking workgroups), cap."""
    c = constants()
    nsegs = rows * ((W + c["kBX"] - 1) // c["kBX"])
    scan = min((nsegs + 255) // 256, 4 * num_cus) * c["kScanSplit"]
    walk = min(4 * num_cus, max(1, nsegs // 16))
    return dict(nsegs=nsegs, scan=scan, walk=walk, cap=young_append_cap(rows, W))


STEPS = (1, 2, 4, 8, 16, 32, 64)


def atrous_table(W: int, rows: int, num_cus: int) -> dict:
    """{step: atrous_lds(...)} for every step the streaming kernel serves."""
    return {S: atrous_lds(W, rows, S, num_cus) for S in STEPS}
