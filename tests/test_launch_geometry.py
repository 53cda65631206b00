"""The host restatement of the streaming kernels' launch geometry (tests/launch_geometry.py), pinned (CPU test; no GPU).

The GPU tests of tests/test_gpu_fullsize_parity.py ask that module whether the launch they check really runs long bands.  Here it is held
to the numbers the documents quote, to the table of the full-size parity issue, and to the
copy of the band rule that tools/uniform_share_emul.py carries (whose emulation matches the device's own counters, tests/test_uniform_share.py)."""
import os
import sys

import pytest

from tests import launch_geometry as LG
from tests.conftest import ROOT

CUS = 256                                       # MI355X


def test_constants_read_from_the_headers():
    c = LG.constants()
    assert (c["kTX"], c["kRS"], c["kRing"], c["kRecBytes"], c["kXcds"]) == (128, 2, 6, 32, 8)
    assert (c["kAtrousOversubscribe"], c["kAtrousMinBand"]) == (4, 8)
    assert (c["kMR"], c["kMRing"], c["kMTX"], c["kMRounds"], c["kMRecBytes"]) == (3, 8, 128, 4, 36)
    assert (c["kFT0"], c["kFReach1"], c["kFT1"], c["kBX"], c["kScanSplit"], c["kYoungShards"]) == (128, 4, 120, 64, 2, 8)
    assert c["atrous_waves"] == {1: 5, 2: 5, 4: 5, 8: 5, 16: 4, 32: 3, 64: 2}
    # workgroups resident per CU: by waves up to step 16, by LDS beyond (the comment at svgf_atrous_lds.h:31-32)
    assert {S: LG.atrous_lds(3840, 2160, S, CUS)["per_cu"] for S in LG.STEPS} == {1: 5, 2: 5, 4: 5, 8: 5, 16: 4, 32: 3, 64: 2}
    assert LG.moments_lds(3840, 2160, CUS)["per_cu"] == 4                        # "LDS: 38.6 KB each, four per CU"
    assert LG.moments_lds(3840, 2160, CUS)["lds"] == 38732


def test_the_numbers_the_documents_quote():
    # 14-row bands at 4K step 1, 18 at step 16, the 8-row floor at 1080p, 52 at 8K
    assert LG.atrous_lds(3840, 2160, 1, CUS)["band"] == 14
    assert LG.atrous_lds(3840, 2160, 16, CUS)["band"] == 18
    assert all(LG.atrous_lds(1920, 1080, S, CUS)["band"] == 8 for S in (1, 2, 4, 8, 16, 32))
    assert LG.atrous_lds(7680, 4320, 1, CUS)["band"] == 52
    # the pair launch's bands: one round of resident workgroups would be 136 rows at 4K, two (the rule) 68
    assert LG.atrous_fused12(3840, 2160, CUS)["band"] == 68
    # young_append_cap: "a quarter of the waves of the rows the context holds (4K: 32 400)" (svgf_kernels.h:19)
    assert LG.young_append_cap(2160, 3840) == 32400


def test_the_table_of_bands():
    """Band rows of the three streaming launches on 256 CUs: small frames (every size an oracle test of test_gpu_parity.py and the sweep's
    oracle kinds use) get the floors; 4K and 8K get long bands."""
    for W, H in ((333, 207), (256, 144), (513, 130), (700, 260), (40, 700), (8191, 47)):
        assert all(LG.atrous_lds(W, H, S, CUS)["band"] == 8 for S in (1, 2, 4, 8, 16)), (W, H)
        assert LG.moments_lds(W, H, CUS)["band"] == 8, (W, H)
        assert LG.atrous_fused12(W, H, CUS)["band"] == 32, (W, H)
    assert {S: LG.atrous_lds(3840, 2160, S, CUS)["band"] for S in LG.STEPS} == {1: 14, 2: 14, 4: 14, 8: 14, 16: 18, 32: 24, 64: 34}
    b8k = {S: LG.atrous_lds(7680, 4320, S, CUS)["band"] for S in LG.STEPS}
    assert b8k == {1: 52, 2: 52, 4: 52, 8: 54, 16: 68, 32: 136, 64: 68}
    assert min(b8k.values()) == 52 and max(b8k.values()) == 136
    assert (LG.moments_lds(1920, 1080, CUS)["band"], LG.moments_lds(3840, 2160, CUS)["band"], LG.moments_lds(7680, 4320, CUS)["band"]) == (8, 16, 64)
    assert (LG.atrous_fused12(1920, 1080, CUS)["band"], LG.atrous_fused12(3840, 2160, CUS)["band"], LG.atrous_fused12(7680, 4320, CUS)["band"]) == (32, 68, 270)


def test_cuts_at_4k():
    """The whole cut at BASELINE's 3840x2160: the partial last bands, the XCD groups and the padding workgroups."""
    g = LG.atrous_table(3840, 2160, CUS)
    assert g[16]["nbands"] == 8 and g[16]["last_band"] == 9                     # 135 decimated rows: 7 x 18 + 9
    assert g[1]["last_band"] == 4 and g[32]["last_band"] == 20 and g[64]["nbands"] == 1
    assert all(g[S]["xgroup"] > 1 for S in LG.STEPS)
    assert (g[1]["padding"], g[2]["padding"]) == (86, 56) and all(g[S]["padding"] == 0 for S in (4, 8, 16, 32, 64))
    for S in LG.STEPS:                                                          # every tile is served, padding workgroups are fewer than a group per XCD
        assert g[S]["blocks"] >= g[S]["tiles"] and g[S]["padding"] < 8 * g[S]["xgroup"]
        assert g[S]["tiles"] == g[S]["xtiles"] * g[S]["nbands"] * S
    y = LG.young_launch(3840, 2160, CUS)
    assert (y["nsegs"], y["scan"], y["walk"]) == (129600, 1014, 1024)
    f = LG.atrous_fused12(3840, 2160, CUS)
    assert (f["nbands"], f["xtiles"], f["blocks"], f["xgroup"], f["last_band"]) == (32, 32, 1024, 8, 52)


def test_xcd_grid():
    assert LG.xcd_grid(1, 16) == (8, 1)
    assert LG.xcd_grid(4650, 16) == (4736, 37)
    for n in (1, 7, 8, 9, 127, 128, 129, 1000, 4680, 5040):
        for xm in (1, 2, 16):
            blocks, xgroup = LG.xcd_grid(n, xm)
            assert blocks >= n and blocks % (8 * xgroup) == 0 and blocks - n < 8 * xgroup


def test_a_large_cu_count_sends_the_checked_launches_to_their_floors():
    """The lever a reviewer pulls to see the GPU tests' geometry asserts trip: with 4096 CUs the launches they check are all at the floors
    (8K step 64 alone keeps 10-row bands)."""
    for W, H in ((3840, 2160), (7680, 4320)):
        assert all(r["band"] == 8 for S, r in LG.atrous_table(W, H, 4096).items() if S < 64 or W < 7680)
        assert LG.moments_lds(W, H, 4096)["band"] == 8 and LG.atrous_fused12(W, H, 4096)["band"] == 32


def test_the_share_emulation_cuts_the_same_bands():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import uniform_share_emul as emul
    finally:
        sys.path.pop(0)
    for W, H in ((3840, 2160), (1920, 1080), (7680, 4320), (4096, 2160), (5120, 2880), (333, 207), (8191, 47)):
        for S in LG.STEPS:
            assert emul.band_rows(W, H, S) == LG.atrous_lds(W, H, S, CUS)["band"], (W, H, S)


def test_drift_is_reported(monkeypatch):
    monkeypatch.setattr(LG, "_FORMS", LG._FORMS + [("svgf_atrous_lds.h", "if (band < kAtrousMinBand) band = 12;")])
    LG.constants.cache_clear()
    try:
        with pytest.raises(LG.GeometryDrift):
            LG.constants()
    finally:
        monkeypatch.undo()
        LG.constants.cache_clear()
