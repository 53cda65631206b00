"""tests/plane_arena.py on a numpy buffer (no GPU): the layout it promises, the fills, and — the point of the exercise — that each of its
checks FIRES on one stray byte and names the right place.  A checker that cannot fail is the gap the arena closes."""
import numpy as np
import pytest

from tests import plane_arena as PA

W, H = 37, 9


def _specs(storage="f32"):
    dt = np.float32 if storage == "f32" else np.float16
    return [("motion", (H, W, 4), np.float32), ("normal", (H, W, 4), np.int16), ("colour", (H, W, 4), dt), ("moments", (H, W, 2), dt),
            ("history", (H, W), np.uint8), ("out", (H, W, 4), dt)]


def _contents(storage="f32", seed=1):
    rng = np.random.default_rng(seed)
    dt = np.float32 if storage == "f32" else np.float16
    return {"motion": rng.uniform(0.1, 4, (H, W, 4)).astype(np.float32), "normal": rng.integers(1, 30000, (H, W, 4)).astype(np.int16),
            "colour": rng.uniform(0.1, 1, (H, W, 4)).astype(dt), "moments": rng.uniform(0.1, 1, (H, W, 2)).astype(dt),
            "history": rng.integers(0, 9, (H, W)).astype(np.uint8)}


def _arena(storage="f32", **kw):
    kw.setdefault("like", {"out": "colour"})
    return PA.Arena(_specs(storage), _contents(storage), device=None, **kw)


@pytest.mark.parametrize("storage", ["f32", "f16"])
@pytest.mark.parametrize("margin_rows", [8, 2 * 64 + 8, 200])
def test_margins_are_at_least_the_derived_size(storage, margin_rows):
    a = _arena(storage, margin_rows=margin_rows)
    for p in a.order:
        want = max(4096, margin_rows * p.W * p.texel)
        assert PA.margin_bytes(p.row_bytes, margin_rows) == want
        assert p.before[1] - p.before[0] >= want and p.before[1] == p.start, p.name
        assert p.after[1] - p.after[0] >= want and p.after[0] == p.end, p.name
    # the margins and the planes tile the arena: no byte belongs to nobody
    spans = sorted(s for p in a.order for s in (p.before, (p.start, p.end), p.after))
    assert spans[0][0] == 0 and spans[-1][1] == a.nbytes
    assert all(x[1] == y[0] for x, y in zip(spans, spans[1:]))
    # texel sizes as include/svgf.h states them
    assert {p.name: p.texel for p in a.order} == {"motion": 16, "normal": 8, "colour": 16 if storage == "f32" else 8,
                                                  "moments": 8 if storage == "f32" else 4, "history": 1, "out": 16 if storage == "f32" else 8}


@pytest.mark.parametrize("storage", ["f32", "f16"])
@pytest.mark.parametrize("k", PA.OFFSETS)
def test_the_offsets_requested_are_the_offsets_obtained(storage, k):
    a = _arena(storage, offsets=k)
    for p in a.order:
        assert a.address_offset(p.name) == (k * p.texel) % PA.ALIGN and p.start % p.texel == 0, p.name
    b = _arena(storage, offsets={"colour": 3, "history": 1, "moments": 1})
    got = {n: b.address_offset(n) for n in b.planes}
    tc, tm = (16, 8) if storage == "f32" else (8, 4)
    assert got == {"motion": 0, "normal": 0, "colour": 3 * tc, "moments": tm, "history": 1, "out": 0}
    if storage == "f16":                            # bases at 8-byte, 4-byte and odd addresses
        assert got["colour"] % 16 == 8 and got["moments"] % 8 == 4 and got["history"] % 2 == 1
    with pytest.raises(AssertionError):
        _arena(storage, offsets=2)


@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_tight_layout_packs_the_planes_back_to_back(storage):
    a = _arena(storage, tight=True, fill="live", offsets={"motion": 1})
    for p, q in zip(a.order, a.order[1:]):
        assert q.start == p.end and p.texel >= q.texel and q.start % q.texel == 0, (p.name, q.name)
        assert p.after == (p.end, p.end) and q.before == (q.start, q.start)
    first, last = a.order[0], a.order[-1]
    assert first.before[1] - first.before[0] >= 4096 and last.after[1] - last.after[0] >= 4096
    assert first.before[0] == 0 and last.after[1] == a.nbytes
    assert a.address_offset(first.name) == first.texel          # the first plane takes its offset, the others follow it
    for n, c in _contents(storage).items():
        assert np.array_equal(a.host(n).view(np.uint8), c.view(np.uint8)), n


@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_views_alias_the_arena_and_start_as_given(storage):
    a = _arena(storage, offsets=3)
    for n, c in _contents(storage).items():
        v = a.view(n)
        assert v.shape == c.shape and np.array_equal(v.view(np.uint8), c.view(np.uint8)), n
    assert PA.is_sentinel_array(a.host("out")).all()             # a plane nobody filled starts as the sentinel
    v = a.view("colour")
    v[2, 3, 1] = 0.5
    assert a.host("colour")[2, 3, 1] == 0.5
    a.assert_margins_intact()


def test_mirror_rows():
    assert PA.mirror_rows(4, 6, "before").tolist() == [0, 1, 2, 3, 3, 2]
    assert PA.mirror_rows(4, 6, "after").tolist() == [3, 2, 1, 0, 0, 1]
    assert PA.mirror_rows(1, 3, "after").tolist() == [0, 0, 0]


@pytest.mark.parametrize("storage", ["f32", "f16"])
@pytest.mark.parametrize("margin_rows", [8, 40])
def test_live_fill_is_the_mirrored_rows(storage, margin_rows):
    a = _arena(storage, fill="live", margin_rows=margin_rows, offsets=1)
    c = _contents(storage)
    for n in ("motion", "normal", "colour", "moments", "out"):
        p = a.planes[n]
        src = c["colour"] if n == "out" else c[n]
        for side, (lo, hi) in (("before", p.before), ("after", p.after)):
            whole = (hi - lo) // p.row_bytes
            assert whole >= margin_rows
            for j in range(whole):                                # the j-th row outwards
                b0 = p.start - (j + 1) * p.row_bytes if side == "before" else p.end + j * p.row_bytes
                row = a.expected[b0:b0 + p.row_bytes]
                k = j % (2 * p.rows)
                k = k if k < p.rows else 2 * p.rows - 1 - k
                want = src[k] if side == "before" else src[p.rows - 1 - k]
                assert np.array_equal(row, np.ascontiguousarray(want).reshape(-1).view(np.uint8)), (n, side, j)
    h = a.planes["history"]
    m = np.concatenate([a.expected[h.before[0]:h.before[1]], a.expected[h.after[0]:h.after[1]]])
    assert (m < 4).any() and (m >= 4).any()                      # both sides of the "young" limit


@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_nan_and_zero_fills(storage):
    a = _arena(storage, fill="nan", offsets=3)
    for p in a.order:
        for lo, hi in (p.before, p.after):
            n = (hi - lo) // p.dtype.itemsize * p.dtype.itemsize
            # typed on the plane's own element grid: the elements next to the plane are whole sentinels
            near = a.expected[hi - n:hi] if (lo, hi) == p.before else a.expected[lo:lo + n]
            assert PA.is_sentinel_array(near.view(p.dtype)).all(), p.name
    col = a.planes["colour"]
    first = a.expected[col.end:col.end + col.texel].view(col.dtype)
    assert np.isnan(first.astype(np.float32)).all()
    z = _arena(storage, fill="zero")
    for p in z.order:
        for lo, hi in (p.before, p.after):
            assert not z.expected[lo:hi].any()


@pytest.mark.parametrize("tight", [False, True])
@pytest.mark.parametrize("fill", PA.FILLS)
def test_margin_check_fires_on_one_stray_byte_and_names_it(fill, tight):
    a = _arena("f16", fill=fill, tight=tight, margin_rows=12, offsets=1)
    a.snapshot_inputs("motion", "normal", "colour", "moments", "history")
    a.check("untouched")
    first, last = a.order[0], a.order[-1]
    # one byte, two rows and five texels before the first plane ...
    at = first.start - 2 * first.row_bytes + 5 * first.texel + 3
    a.buf[at] ^= 0x40
    with pytest.raises(AssertionError, match=rf"margin before plane '{first.name}'.*row -2, column 5, byte 3 ") as e:
        a.assert_margins_intact("case")
    assert e.value.args[0].startswith("case:") and f"arena byte {at}" in e.value.args[0]
    assert a.first_stray()[:4] == (first.name, "before", at, (-2, 5, 3))
    a.buf[at] ^= 0x40
    a.assert_margins_intact()
    # ... and one in the row right after the last plane
    at = last.end + 2 * last.texel
    a.buf[at] ^= 0x01
    with pytest.raises(AssertionError, match=rf"margin after plane '{last.name}'.*row {last.rows}, column 2, byte 0 "):
        a.assert_margins_intact()
    a.buf[at] ^= 0x01
    if not tight:                                             # between two planes: the byte belongs to the nearer plane's margin
        p = a.planes["colour"]
        at = p.end + 3 * p.row_bytes + 7 * p.texel + 1
        a.buf[at] ^= 0x80
        with pytest.raises(AssertionError, match=rf"margin after plane 'colour'.*row {p.rows + 3}, column 7, byte 1 "):
            a.assert_margins_intact()
        a.buf[at] ^= 0x80
        at2 = p.start - 1
        a.buf[at2] ^= 0x80
        a.buf[at + 4] ^= 0x80                                  # two strays: the first in address order is the one named
        with pytest.raises(AssertionError, match=rf"margin before plane 'colour'.*row -1, column {p.W - 1}, byte {p.texel - 1} "):
            a.assert_margins_intact()
        a.buf[at2] ^= 0x80
        a.buf[at + 4] ^= 0x80
    a.check("restored")


@pytest.mark.parametrize("tight", [False, True])
def test_input_check_fires_on_one_stray_byte_and_names_it(tight):
    a = _arena("f32", fill="live", tight=tight, offsets=3)
    a.snapshot_inputs("motion", "normal", "colour", "moments", "history")
    a.view("out")[...] = 0.25                                   # an output may change: it is not in the snapshot
    a.assert_inputs_intact()
    n = a.view("normal")
    n.view(np.uint8).reshape(H, W, 8)[4, 11, 6] ^= 0x02
    with pytest.raises(AssertionError, match=r"input plane 'normal' was written: 1 byte\(s\), the first at row 4, column 11, byte 6 "):
        a.assert_inputs_intact("case")
    assert a.first_changed_input()[0] == "normal" and a.first_changed_input()[2] == (4, 11, 6)
    with pytest.raises(AssertionError):
        a.check()
    n.view(np.uint8).reshape(H, W, 8)[4, 11, 6] ^= 0x02
    a.view("history")[H - 1, W - 1] ^= 1
    with pytest.raises(AssertionError, match=rf"input plane 'history'.*row {H - 1}, column {W - 1}, byte 0 "):
        a.assert_inputs_intact()
    a.view("history")[H - 1, W - 1] ^= 1
    a.check()
    a.assert_margins_intact()                                   # writing planes never trips the margin check


def test_a_nan_payload_change_in_a_margin_is_a_stray_write_too():
    """The margin check compares bytes, not values: a NaN sentinel overwritten by another NaN is caught."""
    a = _arena("f32", fill="nan")
    p = a.planes["colour"]
    a.buf[p.end:p.end + 4] = np.array([np.nan], np.float32).view(np.uint8)
    with pytest.raises(AssertionError, match="margin after plane 'colour'"):
        a.assert_margins_intact()
