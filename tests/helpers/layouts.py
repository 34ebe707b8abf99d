"""Memory layouts of float operands for the layout tests (tests/test_layouts_host.py, tests/test_gpu_layouts.py).

`as_layout(t, kind)` returns (view, backing): `view` equals `t` in value and has the requested layout; `backing` is the buffer
the view lives in, every float of which that the view does not cover holds SENTINEL - a NaN with a fixed payload.
`guards_intact(backing)` asserts afterwards that those floats still carry that bit pattern (compared as int32: a stray write of
0.0, of another NaN or of the same value rounded would all be seen) - and, with `value`, that the view still holds its bits.

    dense               a fresh aligned clone: the control
    row_strided         big[:, :C] of an [R, C + 3] buffer (1-D: big[:, 0] of [R, 4])
    row_skipping        big[::2] of a [2 R, C] buffer
    transposed_storage  t.t().contiguous().t()        (2-D only)
    offset4 / offset8   dense and contiguous, 1 / 2 floats into a flat buffer: data_ptr() % 16 == 4 / 8, is_contiguous()
    expanded            stride 0 in every dimension: only for a tensor whose elements are all equal (grad_out of .sum(), a
                        bias expanded from one value)
"""
import torch

KINDS = ("dense", "row_strided", "row_skipping", "transposed_storage", "offset4", "offset8", "expanded")
AWKWARD = tuple(k for k in KINDS if k != "dense")
SENTINEL_BITS = 0x7FC5A5A5          # a quiet NaN with a payload no arithmetic produces
_PAD = 8                            # sentinel floats before and after an offset view


class Backing:
    """The buffer behind a layout view: `buf` (float32, any shape), `mask` (bool, same shape: True where the view's data lies)."""

    def __init__(self, buf, mask, view):
        self.buf, self.mask, self.view = buf, mask, view
        self.before = view.detach().clone()


def _sentinel(shape, device):
    return torch.full(shape, SENTINEL_BITS, dtype=torch.int32, device=device).view(torch.float32)


def as_layout(t: torch.Tensor, kind: str):
    assert t.dtype == torch.float32 and t.dim() in (1, 2), (t.dtype, t.shape)
    t = t.detach()
    dev = t.device
    if kind == "dense":
        buf = t.clone(memory_format=torch.contiguous_format)
        view, mask = buf, torch.ones_like(buf, dtype=torch.bool)
    elif kind == "row_strided":
        r, c = (t.size(0), t.size(1)) if t.dim() == 2 else (t.size(0), 1)
        buf = _sentinel((r, c + 3), dev)
        mask = torch.zeros(r, c + 3, dtype=torch.bool, device=dev)
        mask[:, :c] = True
        view = buf[:, :c] if t.dim() == 2 else buf[:, 0]
        view.copy_(t)
    elif kind == "row_skipping":
        buf = _sentinel((2 * t.size(0),) + tuple(t.shape[1:]), dev)
        mask = torch.zeros_like(buf, dtype=torch.bool)
        mask[::2] = True
        view = buf[::2]
        view.copy_(t)
    elif kind == "transposed_storage":
        assert t.dim() == 2
        buf = t.t().contiguous()
        view, mask = buf.t(), torch.ones_like(buf, dtype=torch.bool)
    elif kind in ("offset4", "offset8"):
        off = 1 if kind == "offset4" else 2
        # (a base that is 16-byte aligned whatever the allocator gave: the first aligned float of a buffer with slack)
        raw = _sentinel((t.numel() + 2 * _PAD + 4 + off,), dev)
        lead = (-(raw.data_ptr() // 4)) % 4
        buf = raw[lead:]
        assert buf.data_ptr() % 16 == 0
        lo = _PAD + off                                    # _PAD is a multiple of 4: the view starts `off` floats past a boundary
        mask = torch.zeros_like(buf, dtype=torch.bool)
        mask[lo:lo + t.numel()] = True
        view = buf[lo:lo + t.numel()].view(t.shape)
        view.copy_(t)
        assert view.is_contiguous() and (view.numel() == 0 or view.data_ptr() % 16 == 4 * off), view.data_ptr()
    elif kind == "expanded":
        flat = t.reshape(-1)
        assert flat.numel() > 0 and bool((flat.view(torch.int32) == flat.view(torch.int32)[0]).all()), \
            "expanded: every element of the tensor must be the same value"
        buf = _sentinel((1 + 2 * _PAD,), dev)
        mask = torch.zeros_like(buf, dtype=torch.bool)
        mask[_PAD] = True
        buf[_PAD] = flat[0]
        view = buf[_PAD].expand(t.shape)
        assert all(s == 0 for s in view.stride())
    else:
        raise ValueError(f"layout kind {kind!r}: one of {KINDS}")
    assert view.shape == t.shape and torch.equal(view.view(torch.int32) if view.is_contiguous() else view.contiguous().view(torch.int32),
                                                 t.contiguous().view(torch.int32))
    return view, Backing(buf, mask, view)


def carve_out(shape, device, fill_sentinel: bool = True):
    """A dense, 16-byte aligned float32 tensor of `shape` cut from the middle of a larger sentinel-filled buffer (a caller-given
    `out`): (view, backing).  The view itself is sentinel-filled too, so that an element the kernel skips is seen."""
    n = 1
    for s in shape:
        n *= int(s)
    raw = _sentinel((n + 2 * _PAD + 4,), device)
    lead = (-(raw.data_ptr() // 4)) % 4
    buf = raw[lead:]
    mask = torch.zeros_like(buf, dtype=torch.bool)
    mask[_PAD:_PAD + n] = True
    view = buf[_PAD:_PAD + n].view(shape)
    assert view.is_contiguous() and view.data_ptr() % 16 == 0
    return view, Backing(buf, mask, view)


def sentinel_like(shape, device):
    """A dense tensor of sentinels (an `out` that must come back untouched from a refused call)."""
    return _sentinel(tuple(shape), device)


def all_sentinel(t: torch.Tensor) -> bool:
    return bool((t.contiguous().view(torch.int32) == SENTINEL_BITS).all())


def guards_intact(backing: Backing, value: bool = True):
    """Every float of the buffer outside the view still is the sentinel, bit for bit; with `value` the view's own bits are
    unchanged too (a read-only operand)."""
    bits = backing.buf.contiguous().view(torch.int32)
    guard = bits[~backing.mask.contiguous()]
    bad = int((guard != SENTINEL_BITS).sum())
    assert bad == 0, f"{bad} of {guard.numel()} guard floats around the operand were overwritten"
    if value:
        now = backing.view.detach().contiguous().view(torch.int32)
        assert torch.equal(now, backing.before.contiguous().view(torch.int32)), "the read-only operand's own bits changed"
