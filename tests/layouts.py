"""Helpers shared by the layout tests (tests/test_layout_host.py, tests/test_gpu_layouts.py): the pointer fields of a ctypes
argument struct, found from the struct definitions themselves, and tensor layouts -- the same VALUES as a dense view at an element
offset into a larger buffer (a 4- or 8-byte aligned base) or as a non-contiguous view of a base tensor.
"""
from __future__ import annotations

import ctypes as C

import torch


def pointer_fields(obj, prefix=""):
    """Every device-pointer slot of the ctypes structure ``obj``, recursively: yields ``(path, owner, key)`` with ``path`` spelled as
    in include/lightplane_hip.h (``rays.encoding``, ``grid.grids[2].data``, ``grad_grid_list[3]``); ``getattr(owner, key)`` /
    ``owner[key]`` reads the slot.  Driven by ``_fields_``: a ``c_void_p`` field, an array of ``c_void_p``, nested structures and arrays
    of structures.  Any other pointer-like field type raises, so that a field added later in a form this walk does not know cannot
    be skipped silently."""
    for name, tp in obj._fields_:
        val = getattr(obj, name)
        path = prefix + name
        if tp is C.c_void_p:
            yield path, obj, name
        elif isinstance(tp, type) and issubclass(tp, C.Structure):
            yield from pointer_fields(val, path + ".")
        elif isinstance(tp, type) and issubclass(tp, C.Array):
            et = tp._type_
            for i in range(tp._length_):
                if et is C.c_void_p:
                    yield f"{path}[{i}]", val, i
                elif issubclass(et, C.Structure):
                    yield from pointer_fields(val[i], f"{path}[{i}].")
                else:
                    assert issubclass(et, (C.c_int32, C.c_int64, C.c_float, C.c_double)), f"{path}: array of {et}: pointer or not?"
        else:
            assert tp in (C.c_int32, C.c_int64, C.c_float, C.c_double, C.c_int), f"{path}: field type {tp}: pointer or not?"


def get_slot(owner, key):
    return getattr(owner, key) if isinstance(key, str) else owner[key]


def set_slot(owner, key, value):
    if isinstance(key, str):
        setattr(owner, key, value)
    else:
        owner[key] = value


def snapshot(struct):
    """A private copy of a ctypes structure (the wrappers patch and re-use their argument blocks after the call)."""
    return type(struct).from_buffer_copy(struct)


# ---- tensor layouts -------------------------------------------------------------------------------------------------------------

VARIANTS = ("off4", "off8", "strided")


class Layout:
    """``values`` (a dense CPU tensor) laid out inside a larger base tensor.  ``base_cpu`` holds the values where ``view(base)`` looks and
    N(0, 1) junk everywhere else (a kernel or a wrapper that reads the base as if it were dense sees wrong numbers, not zeros).
    ``view`` maps a base tensor (on any device) to the view with the values' shape; ``covered()`` is the boolean mask of the base's
    elements the view covers."""

    identity = False  # (True: the values in a fresh dense tensor of their own -- base and view are the same tensor)

    def __init__(self, values, base_shape, view, seed=0):
        gen = torch.Generator().manual_seed(1234 + seed)
        self.view = view
        if values.dtype.is_floating_point:
            self.base_cpu = torch.randn(*base_shape, generator=gen, dtype=values.dtype)
        else:
            self.base_cpu = torch.zeros(*base_shape, dtype=values.dtype)
        v = view(self.base_cpu)
        assert v.shape == values.shape, (tuple(v.shape), tuple(values.shape))
        v.copy_(values)

    def covered(self):
        m = torch.zeros(self.base_cpu.shape, dtype=torch.bool)
        self.view(m).fill_(True)
        return m

    def on(self, dev, requires_grad=False):
        """(base leaf on ``dev``, the view of it that carries the values)."""
        base = self.base_cpu.to(dev).clone().requires_grad_(requires_grad)
        return base, self.view(base)


def offset_layout(values, elems, seed=0):
    """Contiguous view at an offset of ``elems`` elements into a flat buffer: ``buf[elems : elems + n].view(shape)``."""
    n, shape = values.numel(), tuple(values.shape)
    return Layout(values, (n + 8,), lambda b: b[elems: elems + n].view(shape), seed)


def strided_layout(values, kind, seed=0):
    """Non-contiguous views.  ``kind``: "rows" -- every other row of a tensor twice as long (``big[::2]``; ray fields, flat parameter
    vectors, anything indexed along dim 0); "columns" -- the leading columns of a wider matrix (``wide[:, :E]``); "grid" -- a
    permutation of a tensor stored channels-first (the last dim stored first)."""
    shape = tuple(values.shape)
    if kind == "rows":
        return Layout(values, (2 * shape[0],) + shape[1:], lambda b: b[::2], seed)
    if kind == "columns":
        e = shape[1]
        return Layout(values, (shape[0], e + 3), lambda b: b[:, :e], seed)
    assert kind == "grid" and len(shape) >= 2, kind
    nd = len(shape)
    perm = tuple(range(1, nd)) + (0,)
    return Layout(values, (shape[-1],) + shape[:-1], lambda b: b.permute(*perm), seed)


def identity_layout(values):
    """The values in a fresh dense tensor of their own: what the other GPU tests hand over."""
    lay = Layout(values, tuple(values.shape), lambda b: b)
    lay.identity = True
    return lay


def make_layout(values, variant, kind="rows", seed=0):
    """``kind`` picks the strided view (``strided_layout``) and, besides: "as_is" -- an input the front-end hands to the library as it is
    and refuses in any other layout: fresh in EVERY variant (the refusals have a test of their own); "offset_only" -- an input the
    front-end copies when it is under-aligned but refuses when it is not dense: fresh in the strided variant.  An integer input
    (``ray_grid_idx``) arrives as int32 at the element offset -- int32, so that the front-end's dtype conversion does not realign it by
    accident -- and as every other element of an int64 tensor."""
    if not values.dtype.is_floating_point:
        values = values.to(torch.int64 if variant == "strided" else torch.int32)
    if kind == "as_is" or (kind == "offset_only" and variant == "strided"):
        return identity_layout(values)
    if variant == "off4":
        return offset_layout(values, 1, seed)
    if variant == "off8":
        return offset_layout(values, 2, seed)
    assert variant == "strided", variant
    return strided_layout(values, kind, seed)
