"""Guard bands around operands: pins "an op reads nothing it uses, and writes nothing, outside the extents its arguments declare;
it writes every element it owns".

place() copies an operand into the middle of ONE larger flat allocation and returns a view with the requested row stride plus a handle.
Around the operand lie a lead and a trail band (each >= 64 KiB and >= 256 rows of the operand's stride, a multiple of 256 bytes, so the view
keeps the alignment a tight tensor has); with ld > cols the gap columns of every row belong to the bands.  Every over-read and over-write
this can detect therefore stays inside the allocation: no operand ever lies flush against its end.

What the bands hold, by role:
  input,  float / bf16 / fp16   NaN -- an over-read that is USED (even times a zero weight or a zero probability) poisons the output
  input,  uint8 / bool (masks)  1, "valid" -- an over-read admits a poisoned key or row
  input,  other integers        0.  Over-reads of integer operands (lengths, labels, offsets) are OUTSIDE what this suite claims: a stray
                                zero length or label changes nothing one could tell from a legitimate one.
  output                        the extent is pre-filled with NaN (integers: -1 / 0xFF), so an owned element the op did not write fails the
                                caller's comparison with the reference; bands and gaps hold the byte 0xA5
  inout                         (residual in place, accumulate = 1, optimizer state, rings and caches) the extent holds the real prior data;
                                bands and gaps as for outputs
A workspace whose size the caller takes from a formula in include/cfm.h is an output of exactly that size (workspace()): an overrun of
it becomes a failure.

check() compares bands and gaps (for inputs: the extent too) byte for byte with what was planted and names the first offending offset
relative to the extent as (row, column); negative rows are the lead band, columns >= cols a gap.  What it cannot see: a clamped
over-read whose value is discarded, and integer operands (above).

A 1-D operand counts as n rows of one element (stride 1) when the band size is worked out.  Plain helper module: no fixtures, no session state."""
import torch

MIN_BAND = 64 * 1024
MIN_ROWS = 256
ALIGN = 256
BAND_BYTE = 0xA5


def _round_up(n, m):
    return (n + m - 1) // m * m


class Placed:
    """Handle of one placed operand: .view (what the op gets), .check() (bands, gaps and -- for inputs -- the extent are untouched)."""

    def __init__(self, flat, view, role, lead, rows, cols, ld, esize, name):
        self.flat, self.view, self.role, self.lead, self.rows, self.cols, self.ld, self.esize, self.name = flat, view, role, lead, rows, cols, ld, esize, name
        self.planted = flat.clone()
        if role == "input":
            self.own = None
        else:
            own = torch.zeros(flat.numel(), dtype=torch.bool, device=flat.device)
            ext = own[lead:lead + rows * ld * esize].view(rows, ld * esize)
            ext[:, :cols * esize] = True
            self.own = own

    def check(self):
        diff = self.flat != self.planted
        if self.own is not None:
            diff &= ~self.own
        if bool(diff.any()):
            off = int(torch.nonzero(diff)[0, 0])
            elem = (off - self.lead) // self.esize             # floor: negative in the lead band
            row, col = elem // self.ld, elem % self.ld
            where = "extent" if 0 <= row < self.rows and col < self.cols else "lead band" if row < 0 else "gap" if row < self.rows else "trail band"
            raise AssertionError("%s (%s): byte changed in the %s at row %d, column %d of the extent [%d x %d, stride %d] (%d bytes differ; planted 0x%02x, now 0x%02x)"
                                 % (self.name, self.role, where, row, col, self.rows, self.cols, self.ld, int(diff.sum()), int(self.planted[off]), int(self.flat[off])))


def _band_bytes(ld, esize, want):
    return _round_up(max(MIN_BAND, MIN_ROWS * ld * esize, want or 0), ALIGN)


def _place(shape, dtype, device, data, ld, lead, trail, role, name):
    assert role in ("input", "output", "inout"), role
    shape = tuple(int(s) for s in shape)
    esize = torch.empty((), dtype=dtype).element_size()
    if len(shape) <= 1:
        n = shape[0] if shape else 1
        rows, cols, ld, band_ld = 1, n, max(n, 1), 1
    else:
        cols = shape[-1]
        rows = 1
        for s in shape[:-1]:
            rows *= s
        ld = cols if ld is None else int(ld)
        band_ld = ld
        assert ld >= cols, "row stride %d below the %d columns" % (ld, cols)
    lead_b, trail_b = _band_bytes(band_ld, esize, lead), _band_bytes(band_ld, esize, trail)
    body = _round_up(max(rows * ld * esize, 1), ALIGN)
    flat = torch.empty(lead_b + body + trail_b, dtype=torch.uint8, device=device)
    raw = torch.uint8 if dtype == torch.bool else dtype
    typed = flat.view(raw)
    if role == "input":
        if dtype.is_floating_point:
            typed.fill_(float("nan"))
        else:
            typed.fill_(1 if dtype in (torch.uint8, torch.bool) else 0)
    else:
        flat.fill_(BAND_BYTE)
    vshape = shape if shape else (1,)
    strides = [1] * len(vshape)
    if len(vshape) > 1:
        strides[-2] = ld
        for i in range(len(vshape) - 3, -1, -1):
            strides[i] = strides[i + 1] * vshape[i + 1]
    view = typed.as_strided(vshape, strides, lead_b // esize)
    if data is not None:
        view.copy_(data.view(raw) if dtype == torch.bool else data)
    elif dtype.is_floating_point:
        view.fill_(float("nan"))
    else:
        view.fill_(0xFF if dtype in (torch.uint8, torch.bool) else -1)
    if not shape:
        view = view.view(())
    return view, Placed(flat, view, role, lead_b, rows, cols, ld, esize, name or "operand")


def place(t, ld=None, lead=None, trail=None, role="input", name=None):
    """Copy `t` (any rank, last axis contiguous) into a guarded allocation; rows (all axes but the last, flattened) are `ld` elements apart.
    role "input" | "inout" | "output" (t gives shape / dtype / device only).  Returns (view, handle)."""
    return _place(t.shape, t.dtype, t.device, None if role == "output" else t, ld, lead, trail, role, name)


def out(shape, dtype, device, ld=None, lead=None, trail=None, name=None):
    """A guarded output of this shape: extent NaN (integers -1 / 0xFF), bands and gaps 0xA5.  Returns (view, handle)."""
    return _place(shape, dtype, device, None, ld, lead, trail, "output", name)


def workspace(numel, dtype, device, name=None):
    """A workspace of EXACTLY the documented size, guarded like an output."""
    return _place((int(numel),), dtype, device, None, None, None, None, "output", name or "workspace")


class Guards:
    """The operands of one call: g.inp(t) / g.io(t) / g.out(shape, dtype) / g.ws(n) return views; g.check() checks every handle."""

    def __init__(self, device="cuda"):
        self.device, self.handles = device, []

    def _keep(self, pair):
        self.handles.append(pair[1])
        return pair[0]

    def inp(self, t, ld=None, name=None, **kw):
        return None if t is None else self._keep(place(t.to(self.device), ld, role="input", name=name, **kw))

    def io(self, t, ld=None, name=None, **kw):
        return self._keep(place(t.to(self.device), ld, role="inout", name=name, **kw))

    def out(self, shape, dtype=torch.float32, ld=None, name=None, **kw):
        return self._keep(out(shape, dtype, self.device, ld, name=name, **kw))

    def ws(self, numel, dtype=torch.float32, name=None):
        return self._keep(workspace(numel, dtype, self.device, name))

    def check(self):
        for h in self.handles:
            h.check()
