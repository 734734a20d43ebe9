"""Poisoned, fenced allocations for the buffers the front-ends hand to the kernels (tests/test_guarded_alloc_host.py proves the harness,
tests/test_gpu_unwritten_buffers.py runs every kernel file under it).

include/lightplane_hip.h promises of every buffer either that the kernel WRITES every element (the front-ends allocate those with
``torch.empty`` / ``torch.empty_like``) or that it ACCUMULATES into a buffer the caller zero-filled (``torch.zeros`` /
``torch.zeros_like``).  An oracle comparison cannot see a broken promise: it reads its results out of memory whose earlier contents
nobody controlled -- the caching allocator hands back the block the same test wrote a moment ago, a fresh block is zero.

``guarded(pattern)`` replaces the four module attributes ``torch.empty``, ``torch.empty_like``, ``torch.zeros`` and
``torch.zeros_like`` (the attributes themselves, not a per-thread copy: autograd runs a backward on a thread of its own) for the
duration of the block.  For a device tensor of dtype float32 / float64 / int32 / int64 / uint8 the replacement

* allocates the payload between two FENCES of ``FENCE_BYTES`` = 256 bytes (a multiple of the 16 bytes the library asks of a base
  pointer, so ``_lib.aligned`` makes no copy) filled with the byte ``CANARY``;
* fills the payload with the POISON of the current pattern (``empty``, ``empty_like``) or with zeros (``zeros``, ``zeros_like``);
* records ``(call site, shape, dtype, fences, payload)`` in the ledger.

Anything else -- a CPU tensor, another dtype, ``out=``, a non-contiguous ``memory_format``, a layout, pinned memory -- goes to the real
function unchanged; a request of zero elements goes there as well, but is recorded.

``check()`` (also run when the block ends without an exception) requires every fence to be bit-identical to the canary still and
names call site and byte offset otherwise; ``unwritten(record)`` counts the payload elements that still hold the poison's bit pattern.

Patterns (``PATTERNS``).  A stale value is rarely a NaN: it is what the previous owner of the block left, a plausible number.  And a
NaN alone can be swallowed -- ``if (!(nlt > 0.0f)) nlt = 0`` behind the tuned backward's checkpoint read turns a NaN and any negative
garbage into a plausible 0 -- so the set holds a NaN, a huge positive, a huge negative and a plausible value:

    name     float32 / float64                 int32 / int64    uint8
    nan      quiet NaN (mantissa tagged)       -1               255
    +1e30    +1e30                             123456789        165
    -1e30    -1e30                             123456789        165
    0.5      0.5                               123456789        165

(the NaN carries a mantissa tag so that a NaN a kernel computes or copies from its input -- 0x7fc00000 -- is not taken for poison).
The canary byte 0xC3 repeats to -391.53 (float32), about -2.8e15 (float64), 0xC3C3C3C3 (integers) and 195 (uint8): none of the poisons.
"""
from __future__ import annotations

import contextlib
import linecache
import math
import os
import re
import struct
import sys
import threading
from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch

FENCE_BYTES = 256
CANARY = 0xC3
PATTERNS = ("nan", "+1e30", "-1e30", "0.5")

_NAN32 = 0x7FC0DEAD          # quiet NaN, tagged
_NAN64 = 0x7FF8DEAD0000BEEF
_FLOAT = {"+1e30": 1e30, "-1e30": -1e30, "0.5": 0.5}
_INT = {"nan": -1}           # every other pattern: _INT_OTHER
_INT_OTHER = 123456789
_U8 = {"nan": 255}
_U8_OTHER = 165
_BITS_VIEW = {torch.float32: torch.int32, torch.float64: torch.int64, torch.int32: torch.int32, torch.int64: torch.int64,
              torch.uint8: torch.uint8}
GUARDED_DTYPES = tuple(_BITS_VIEW)
_HERE = os.path.abspath(__file__)
_TORCH_DIR = os.path.dirname(os.path.abspath(torch.__file__)) + os.sep
_NAMES = ("empty", "empty_like", "zeros", "zeros_like")


def _signed(bits: int, width: int) -> int:
    return bits - (1 << width) if bits >= 1 << (width - 1) else bits


def poison_bits(pattern: str, dtype: torch.dtype) -> int:
    """The poison of ``pattern`` for ``dtype`` as the integer its bits spell in ``_BITS_VIEW[dtype]``."""
    assert pattern in PATTERNS, f"unknown poison pattern {pattern!r} (known: {PATTERNS})"
    if dtype == torch.float32:
        return _signed(_NAN32, 32) if pattern == "nan" else struct.unpack("<i", struct.pack("<f", _FLOAT[pattern]))[0]
    if dtype == torch.float64:
        return _signed(_NAN64, 64) if pattern == "nan" else struct.unpack("<q", struct.pack("<d", _FLOAT[pattern]))[0]
    if dtype in (torch.int32, torch.int64):
        return _INT.get(pattern, _INT_OTHER)
    if dtype == torch.uint8:
        return _U8.get(pattern, _U8_OTHER)
    raise TypeError(f"{dtype} is not a guarded dtype")


@dataclass
class Record:
    """One allocation made inside ``guarded``."""
    fn: str                                  # "empty", "empty_like", "zeros", "zeros_like"
    site: Tuple[str, int, str]               # (file, line, function) of the caller outside torch and this module
    shape: Tuple[int, ...]
    dtype: torch.dtype
    fences: Optional[Tuple[torch.Tensor, torch.Tensor]]   # uint8 views in front of and behind the payload; None: not fenced
    payload: torch.Tensor
    pattern: str

    @property
    def poisoned(self) -> bool:
        return self.fences is not None and self.fn in ("empty", "empty_like")

    @property
    def name(self) -> str:
        """The variable the call site assigns (``ckpt = torch.empty(...)`` -> "ckpt"), or "" where the line is no plain assignment."""
        m = re.match(r"\s*([A-Za-z_][\w, ]*?)\s*=[^=]", linecache.getline(self.site[0], self.site[1]))
        return m.group(1) if m else ""

    def where(self) -> str:
        return f"torch.{self.fn} at {self.site[0]}:{self.site[1]} ({self.site[2]}), shape {self.shape}, {self.dtype}"


def _call_site() -> Tuple[str, int, str]:
    f = sys._getframe(2)
    while f is not None:
        fn = os.path.abspath(f.f_code.co_filename)
        if fn != _HERE and not fn.startswith(_TORCH_DIR) and not fn.endswith("contextlib.py"):
            return (fn, f.f_lineno, f.f_code.co_name)
        f = f.f_back
    return ("?", 0, "?")


def _size_of(args, kwargs):
    if "size" in kwargs:
        size = kwargs.pop("size")
    elif len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        size = args[0]
    else:
        size = args
    return tuple(int(s) for s in size)


class Guard:
    def __init__(self, pattern: str, device: str = "cuda"):
        assert pattern in PATTERNS, f"unknown poison pattern {pattern!r} (known: {PATTERNS})"
        self.pattern = pattern
        self.device_type = device       # "cpu": the switch of tests/test_guarded_alloc_host.py, where torch code stands in for a kernel
        self.records: List[Record] = []
        self._lock = threading.Lock()
        self._real = {}

    # ---- allocation ---------------------------------------------------------------------------------------------------------------
    def _allocate(self, fn, shape, dtype, device, requires_grad):
        real_empty = self._real["empty"]
        n = math.prod(shape)
        nbytes = n * real_empty(0, dtype=dtype).element_size()
        fence = FENCE_BYTES
        raw = real_empty(fence + nbytes + fence, dtype=torch.uint8, device=device)
        payload = raw[fence:fence + nbytes].view(dtype).view(shape)
        if fn in ("zeros", "zeros_like"):
            payload.zero_()
        else:
            payload.view(-1).view(_BITS_VIEW[dtype]).fill_(poison_bits(self.pattern, dtype))
        fences = (raw[:fence], raw[fence + nbytes:])
        fences[0].fill_(CANARY)
        fences[1].fill_(CANARY)
        rec = Record(fn, _call_site_cache.site, shape, dtype, fences, payload, self.pattern)
        with self._lock:
            self.records.append(rec)
        return payload.requires_grad_() if requires_grad else payload

    def _make(self, fn):
        real = self._real[fn]
        like = fn.endswith("_like")
        guard = self

        def replacement(*args, **kwargs):
            try:
                kw = dict(kwargs)
                if like:
                    src = args[0] if args else kw.pop("input")
                    if len(args) > 1 or not torch.is_tensor(src):
                        return real(*args, **kwargs)
                    shape = tuple(src.shape)
                    dtype = kw.pop("dtype", None) or src.dtype
                    device = kw.pop("device", None)
                    device = src.device if device is None else torch.device(device)
                    mf = kw.pop("memory_format", torch.preserve_format)
                    plain = mf == torch.contiguous_format or (mf == torch.preserve_format and src.is_contiguous())
                    if src.layout != torch.strided:
                        plain = False
                else:
                    shape = _size_of(args, kw)
                    dtype = kw.pop("dtype", None) or torch.get_default_dtype()
                    device = kw.pop("device", None)
                    device = guard._real["empty"](0).device if device is None else torch.device(device)
                    plain = kw.pop("memory_format", torch.contiguous_format) == torch.contiguous_format
                requires_grad = bool(kw.pop("requires_grad", False))
            except Exception:
                return real(*args, **kwargs)   # (whatever is wrong with the call: the real function says it)
            if kw or not plain or device.type != guard.device_type or dtype not in GUARDED_DTYPES:
                return real(*args, **kwargs)
            _call_site_cache.site = _call_site()
            if math.prod(shape) == 0:   # nothing to poison or to fence: forwarded, but on the ledger
                out = real(*args, **kwargs)
                with guard._lock:
                    guard.records.append(Record(fn, _call_site_cache.site, shape, dtype, None, out, guard.pattern))
                return out
            return guard._allocate(fn, shape, dtype, device, requires_grad)

        replacement.__name__ = f"guarded_{fn}"
        return replacement

    def __enter__(self):
        self._real = {n: getattr(torch, n) for n in _NAMES}
        for n in _NAMES:
            setattr(torch, n, self._make(n))
        return self

    def __exit__(self, exc_type, exc, tb):
        for n in _NAMES:
            setattr(torch, n, self._real[n])
        if exc_type is None:
            self.check()
        return False

    # ---- checks -------------------------------------------------------------------------------------------------------------------
    def fence_failures(self) -> List[str]:
        out = []
        for r in self.records:
            if r.fences is None:
                continue
            for side, f in zip(("before", "behind"), r.fences):
                bad = (f != CANARY).nonzero()
                if bad.numel():
                    k = int(bad[0])
                    # offsets count from the payload's ends: -1 is the byte in front of the first element, +0 the byte behind the last
                    off = k - f.numel() if side == "before" else k
                    out.append(f"fence {side} the payload overwritten at byte offset {off:+d} ({int(bad.numel())} of {f.numel()} bytes): "
                               f"{r.where()}")
        return out

    def check(self):
        """Every fence is bit-identical to the canary."""
        bad = self.fence_failures()
        assert not bad, "; ".join(bad)

    def unwritten_mask(self, r: Record) -> torch.Tensor:
        assert r.poisoned, f"not a poisoned buffer: {r.where()}"
        return r.payload.detach().reshape(-1).view(_BITS_VIEW[r.dtype]) == poison_bits(r.pattern, r.dtype)

    def unwritten(self, r: Record) -> int:
        """Elements of the payload that still hold the poison's bit pattern."""
        return int(self.unwritten_mask(r).sum())

    def from_file(self, suffix: str) -> List[Record]:
        """The records whose call site is in a file whose path ends in ``suffix``."""
        suffix = suffix.replace("/", os.sep)
        return [r for r in self.records if r.site[0].endswith(suffix)]


_call_site_cache = threading.local()


@contextlib.contextmanager
def guarded(pattern: str, device: str = "cuda"):
    """``with guarded("nan") as g: ...`` -- see the module docstring.  ``device="cpu"`` exists for the harness's own test
    (tests/test_guarded_alloc_host.py), where plain torch code stands in for a kernel."""
    g = Guard(pattern, device)
    with g:
        yield g
