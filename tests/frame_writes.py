"""Guarded, poisoned frame buffers: does a render write every float of its target, and nothing beside it?  Plain module, no fixtures:
tests/test_frame_writes.py shows on any machine that the checker names each kind of defect, tests/test_frame_writes_gpu.py renders into it.

One flat allocation holds  guard | rows x width x 3 items | guard  (+ a few items of slack for the alignment).  A guard is GUARD_ROWS rows of
the frame plus GUARD_EXTRA items: more than one block row (16 rows) of overshoot, whichever way.  The frame starts on a 16-byte boundary or
4 bytes behind one (a legal caller buffer: the 16-byte writers of tile_device.h and k_compose test the address and must take their scalar
branch).  Before every call the WHOLE allocation is overwritten, through an integer view so that the bits are exact, with one of

  "nan"    0x7FC0DEAD, a quiet NaN with a recognisable payload.  It survives a read-modify-write (x + NaN, NaN / spp keep the payload's NaN), and
           no scene of the tests computes a NaN, so any NaN in a frame is poison that was read or left;
  "neg"    -1.0, as the pipelined tests fill their buffers;
  "stale"  the frame of ANOTHER camera of the same scene and size between guards of 0x7FC0DEAD: what a real caller's buffer holds.  A float
           of it that survives cannot be told from a pixel by itself (the two cameras share their background): this poison shows in the
           comparison of the frame with the other two poisons' frames, bit for bit (first_difference).

check() reports the first offending index and value of: a guard item that is not bit-identical to its poison; a frame float that still
carries the poison's bits; a padding row (the rows of a tiled frame's compact buffer past the owner's last real row, nrays_tile_rows minus
the rows owned: include/nrays_abi.h, NraysRenderParams::band_rows) that is not exactly +0.0.  It returns the frame as well.
Byte frames (nrays_render_rgb8): the poisons are the bytes 0xAD / 0x52; a byte of a frame may legitimately equal either, so "left over" is
again decided by comparing the two poisons' frames."""
import numpy as np

NAN_BITS = 0x7FC0DEAD
NEG_BITS = 0xBF800000  # -1.0f
POISONS = ("nan", "neg", "stale")
BYTE_POISON = {"nan": 0xAD, "neg": 0x52}
GUARD_ROWS, GUARD_EXTRA, SLACK = 16, 64, 32


def _i32(bits):
    """The int32 that holds `bits` (fill values of int32 views)."""
    return int(np.array([bits], dtype=np.uint32).view(np.int32)[0])


def owned_rows(height, band_rows, band_owner, band_owners):
    """Real rows of an owner's compact buffer (the bands b with b % band_owners == band_owner, clipped to the frame)."""
    if band_rows == 0 or band_owners <= 1:
        return height
    return sum(1 for j in range(height) if (j // band_rows) % band_owners == band_owner)


class Layout:
    """guard | rows * width * channels items | guard; the last pad_rows rows of the frame are padding rows."""

    def __init__(self, rows, width, pad_rows=0, channels=3):
        assert 0 <= pad_rows <= rows
        self.rows, self.width, self.pad_rows, self.channels = rows, width, pad_rows, channels
        self.guard = GUARD_ROWS * width * channels + GUARD_EXTRA  # a multiple of 16 items: the frame is aligned as the first guard is
        self.n = rows * width * channels
        self.items = self.guard + self.n + self.guard + SLACK

    @classmethod
    def of_params(cls, lib, p):
        """The compact buffer of a render with params `p`: rows from nrays_tile_rows, padding rows = those rows minus the rows owned."""
        import ctypes as C
        rows = int(lib.nrays_tile_rows(C.byref(p)))
        return cls(rows, p.width, rows - owned_rows(p.height, p.band_rows, p.band_owner, p.band_owners))

    def frame_at(self, address, itemsize, misaligned):
        """Index of the frame's first item in an allocation that starts at `address`: 16-byte aligned, or 4 bytes behind such a boundary."""
        want = 4 if misaligned else 0
        skip = (want - address - self.guard * itemsize) % 16
        assert skip % itemsize == 0 and skip // itemsize < SLACK
        at = skip // itemsize + self.guard
        assert (address + at * itemsize) % 16 == want
        return at


class Report:
    """What check() found.  guard / leftover / padding: None, or (index, bits) of the first offender — a guard's index counts from the
    frame's first item (negative: before the frame; >= n: behind it), the other two are indices into the frame."""

    def __init__(self, frame, guard, leftover, padding):
        self.frame, self.guard, self.leftover, self.padding = frame, guard, leftover, padding

    def problems(self):
        out = []
        if self.guard is not None:
            out.append("guard overwritten at frame index %d: 0x%08X" % self.guard)
        if self.leftover is not None:
            out.append("poison left in the frame at index %d: 0x%08X" % self.leftover)
        if self.padding is not None:
            out.append("padding row not +0.0 at frame index %d: 0x%08X" % self.padding)
        return out


def _first(mask):
    k = np.flatnonzero(mask)
    return None if k.size == 0 else int(k[0])


def check(alloc, at, layout, poison):
    """alloc: the whole allocation after the call, as a flat unsigned array (uint32 for float frames, uint8 for byte frames); at: index of the
    frame's first item; poison: "nan" / "neg" / "stale"."""
    alloc = np.ascontiguousarray(alloc).reshape(-1)
    byte = alloc.dtype == np.uint8
    assert byte or alloc.dtype == np.uint32
    assert alloc.size == layout.items
    n = layout.n
    if byte:
        guard_bits = frame_bits = BYTE_POISON[poison]
    else:
        guard_bits = NAN_BITS if poison in ("nan", "stale") else NEG_BITS
        frame_bits = None if poison == "stale" else guard_bits
    outside = np.ones(alloc.size, dtype=bool)
    outside[at:at + n] = False
    g = _first(outside & (alloc != guard_bits))
    guard = None if g is None else (g - at, int(alloc[g]))
    body = alloc[at:at + n].copy()
    leftover = None
    if frame_bits is not None and not byte:
        k = _first(body == frame_bits)
        leftover = None if k is None else (k, int(body[k]))
    padding = None
    if layout.pad_rows:
        first_pad = (layout.rows - layout.pad_rows) * layout.width * layout.channels
        k = _first(body[first_pad:] != 0)  # +0.0 is all bits clear
        padding = None if k is None else (first_pad + k, int(body[first_pad + k]))
    frame = (body if byte else body.view(np.float32)).reshape(layout.rows, layout.width, layout.channels)
    return Report(frame, guard, leftover, padding)


def first_difference(a, b):
    """None if the two frames are bit-identical, else (index, bits of a, bits of b) of the first float (byte) that differs."""
    a, b = np.ascontiguousarray(a).reshape(-1), np.ascontiguousarray(b).reshape(-1)
    assert a.shape == b.shape and a.dtype == b.dtype
    if a.dtype == np.float32:
        a, b = a.view(np.uint32), b.view(np.uint32)
    k = _first(a != b)
    return None if k is None else (k, int(a[k]), int(b[k]))


class HostBuffer:
    """The guarded allocation in host memory: float32 frames (nrays_render) or uint8 frames (nrays_render_rgb8)."""

    def __init__(self, layout, misaligned, dtype=np.float32):
        self.layout, self.byte = layout, np.dtype(dtype) == np.uint8
        self.bits = np.empty(layout.items, dtype=np.uint8 if self.byte else np.uint32)
        self.at = layout.frame_at(self.bits.ctypes.data, self.bits.itemsize, misaligned)

    @property
    def address(self):
        return self.bits.ctypes.data + self.at * self.bits.itemsize

    def frame_view(self):
        """The frame's items inside the allocation, writable (float32 or uint8, flat)."""
        v = self.bits[self.at:self.at + self.layout.n]
        return v if self.byte else v.view(np.float32)

    def alloc_view(self):
        """The whole allocation, writable, with the frame's first item at index self.at."""
        return self.bits if self.byte else self.bits.view(np.float32)

    def poison(self, kind, stale=None):
        if self.byte:
            self.bits[:] = BYTE_POISON[kind]
            return
        self.bits[:] = NEG_BITS if kind == "neg" else NAN_BITS
        if kind == "stale":
            self.frame_view()[:] = np.ascontiguousarray(stale, dtype=np.float32).reshape(-1)

    def check(self, kind):
        return check(self.bits, self.at, self.layout, kind)


class DeviceBuffer:
    """The guarded allocation in device memory (a torch int32 tensor; `address` is what the library gets as `out`)."""

    def __init__(self, layout, misaligned):
        import torch
        self.layout = layout
        self.bits = torch.empty(layout.items, dtype=torch.int32, device="cuda")
        self.at = layout.frame_at(self.bits.data_ptr(), 4, misaligned)

    @property
    def address(self):
        return self.bits.data_ptr() + 4 * self.at

    def poison(self, kind, stale=None, stream=None):
        """Overwrites the whole allocation on `stream` (a torch stream; None: the current one, which is the null stream unless the caller changed
        it).  stale: the other camera's frame as a float32 CUDA tensor of the frame's size."""
        import torch
        with torch.cuda.stream(stream):
            self.bits.fill_(_i32(NEG_BITS if kind == "neg" else NAN_BITS))
            if kind == "stale":
                self.bits[self.at:self.at + self.layout.n].copy_(stale.reshape(-1).view(torch.int32))

    def check(self, kind):
        """Reads the allocation back (the caller has synchronised, or relies on this copy being ordered behind its stream)."""
        return check(self.bits.cpu().numpy().view(np.uint32), self.at, self.layout, kind)
