"""The checker of tests/frame_writes.py is not vacuous: numpy "renderers" with one defect each — a float left unwritten, a write one float
before / behind the frame, `out += x` for `out = x`, a padding row left alone — are each named by it, and a correct renderer passes under
every poison at both alignments.  No GPU."""
import numpy as np
import pytest

from tests import frame_writes as fw

W, ROWS, PAD = 13, 7, 2  # 13 * 3 is no multiple of 4; the last two rows are padding rows


def _image():
    """Finite, non-zero, none of it equal to a poison."""
    return (np.arange(ROWS * W * 3, dtype=np.float32) * np.float32(0.0078125) + np.float32(0.25)).reshape(ROWS, W, 3)


def _render(buf, defect=None):
    """Writes _image() (padding rows: +0.0) into the frame of `buf` as a renderer with `defect` would."""
    lay, out, at = buf.layout, buf.alloc_view(), buf.at
    img = _image()
    img[ROWS - lay.pad_rows:] = 0.0
    flat = img.reshape(-1)
    real = (ROWS - lay.pad_rows) * W * 3
    if defect == "accumulates":
        out[at:at + lay.n] += flat
        return
    out[at:at + lay.n] = flat
    if defect == "one float unwritten":
        buf.bits[at + 100] = _POISONED[0]
    elif defect == "writes before the frame":
        out[at - 1] = 0.5
    elif defect == "writes behind the frame":
        out[at + lay.n] = 0.5
    elif defect == "padding row untouched":
        buf.bits[at + real + W * 3:at + lay.n] = _POISONED[0]


_POISONED = [0]  # what the allocation held before the call (the "unwritten" defects put it back)


def _run(kind, misaligned, defect=None, pad=PAD):
    buf = fw.HostBuffer(fw.Layout(ROWS, W, pad), misaligned)
    stale = _image()[::-1] * np.float32(3.0)
    buf.poison(kind, stale)
    _POISONED[0] = int(buf.bits[buf.at + 100]) if defect == "one float unwritten" else int(buf.bits[buf.at + buf.layout.n - 1])
    _render(buf, defect)
    return buf.check(kind)


@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "plus4"])
def test_a_correct_renderer_passes_under_every_poison(misaligned):
    frames = {}
    for kind in fw.POISONS:
        rep = _run(kind, misaligned)
        assert rep.problems() == [], (kind, rep.problems())
        frames[kind] = rep.frame
    assert fw.first_difference(frames["nan"], frames["neg"]) is None and fw.first_difference(frames["nan"], frames["stale"]) is None
    want = _image()
    want[ROWS - PAD:] = 0.0
    assert fw.first_difference(frames["nan"], want) is None


@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "plus4"])
def test_the_frame_starts_where_asked(misaligned):
    for dtype in (np.float32, np.uint8):
        buf = fw.HostBuffer(fw.Layout(ROWS, W), misaligned, dtype)
        assert buf.address % 16 == (4 if misaligned else 0)
        assert buf.at >= buf.layout.guard and buf.layout.items - buf.at - buf.layout.n >= buf.layout.guard
    assert fw.Layout(111, 173).guard == 16 * 173 * 3 + 64


@pytest.mark.parametrize("kind", ["nan", "neg"])
def test_one_float_left_unwritten_is_named(kind):
    rep = _run(kind, False, "one float unwritten")
    assert rep.guard is None and rep.padding is None
    assert rep.leftover == (100, fw.NAN_BITS if kind == "nan" else fw.NEG_BITS)
    assert len(rep.problems()) == 1 and "index 100" in rep.problems()[0]


def test_a_stale_float_shows_in_the_comparison():
    """Under "stale" a surviving float looks like a pixel: the frame differs from the other poisons' frames exactly there."""
    rep, good = _run("stale", False, "one float unwritten"), _run("nan", False)
    assert rep.problems() == []
    diff = fw.first_difference(rep.frame, good.frame)
    assert diff is not None and diff[0] == 100


@pytest.mark.parametrize("kind", fw.POISONS)
@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "plus4"])
def test_writes_beside_the_frame_are_named(kind, misaligned):
    half = int(np.array([0.5], dtype=np.float32).view(np.uint32)[0])
    rep = _run(kind, misaligned, "writes before the frame")
    assert rep.guard == (-1, half) and rep.leftover is None and rep.padding is None
    rep = _run(kind, misaligned, "writes behind the frame")
    assert rep.guard == (ROWS * W * 3, half) and rep.leftover is None and rep.padding is None


def test_accumulating_for_assigning_is_named():
    """`out += x`: under "nan" the sum keeps the NaN, under "neg" and "stale" it is a finite wrong number — the three frames differ, and so
    does each from the frame of an assigning renderer."""
    reps = {kind: _run(kind, False, "accumulates", pad=0) for kind in fw.POISONS}
    good = _run("nan", False, pad=0)
    assert np.isnan(reps["nan"].frame).all()
    assert reps["neg"].problems() == [] and reps["stale"].problems() == []  # neither leaves a poison behind: only the comparison shows it
    assert fw.first_difference(reps["nan"].frame, reps["neg"].frame) is not None
    assert fw.first_difference(reps["neg"].frame, reps["stale"].frame) is not None
    for kind in fw.POISONS:
        assert fw.first_difference(reps[kind].frame, good.frame) is not None, kind


@pytest.mark.parametrize("kind", fw.POISONS)
def test_a_padding_row_left_alone_is_named(kind):
    rep = _run(kind, False, "padding row untouched")
    first = (ROWS - PAD + 1) * W * 3  # the second of the two padding rows
    assert rep.padding is not None and rep.padding[0] == first and rep.padding[1] != 0
    assert rep.guard is None
    # minus zero is not what the padding rows hold either
    buf = fw.HostBuffer(fw.Layout(ROWS, W, PAD), False)
    buf.poison(kind, _image())
    _render(buf)
    buf.frame_view()[first + 2] = np.float32(-0.0)
    assert buf.check(kind).padding == (first + 2, 0x80000000)


def test_padding_rows_are_counted_from_the_bands():
    assert fw.owned_rows(111, 0, 0, 1) == 111
    assert [fw.owned_rows(111, 16, o, 3) for o in range(3)] == [47, 32, 32]  # bands 0 3 6 (the ragged one) / 1 4 / 2 5
    assert fw.owned_rows(111, 1, 1, 2) == 55


def test_byte_frames():
    """nrays_render_rgb8: guards in bytes; a byte left alone shows when the two poisons' frames are compared."""
    frames = {}
    for kind in ("nan", "neg"):
        buf = fw.HostBuffer(fw.Layout(ROWS, W), True, np.uint8)
        buf.poison(kind)
        buf.frame_view()[:] = np.arange(ROWS * W * 3) % 251
        assert buf.check(kind).problems() == []
        buf.alloc_view()[buf.at - 1] = 7
        assert buf.check(kind).guard == (-1, 7)
        buf.poison(kind)
        buf.frame_view()[:50] = 9
        buf.frame_view()[51:] = 9
        frames[kind] = buf.check(kind).frame
    assert fw.first_difference(frames["nan"], frames["neg"]) == (50, 0xAD, 0x52)
