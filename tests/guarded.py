"""Guarded, poisoned buffers for the kernels that carve workspaces and write
capacity-limited outputs.

torch's caching allocator rounds every block up and hands out recycled memory,
so a kernel that writes a few bytes past its buffer, or reads a workspace word
it never wrote, passes a test on plain torch tensors.  Here every buffer a kernel
sees is a view into one allocation (the Arena):

  * the view has exactly the bytes requested, at a 256-byte-aligned offset;
  * a canary strip lies on each side: at least 4096 bytes and at least one
    leading-dimension stride of the view (one output row, one workspace slot),
    so an index that is off by one row lands in canary, not in a neighbour;
  * the canary is position-dependent (no two neighbouring bytes, words or
    256-byte pages are alike), so a kernel that stores a constant -- the
    canary's own value at some position included -- is still seen wherever it
    stores more than that one byte;
  * the view is pre-filled with 0x00, with 0xFF (floats NaN, int32 -1, every
    mask word all-ones), or left as the previous call in that carve left it.

Every carve lies inside the one live allocation with its trailing strip, so a
kernel that overruns is reported by check(); it does not fault.

Works on CPU tensors too (tests/test_guarded_cpu.py tests the harness itself).
"""
import sys

import numpy as np
import torch

ZERO = 0x00
ONES = 0xFF
KEEP = None  # leave what the previous call in that carve wrote
FILLS = (ZERO, ONES)

ALIGN = 256
MIN_STRIP = 4096
_PERIOD = 1 << 16


def _round_up(n, a=ALIGN):
    return (int(n) + a - 1) // a * a


def _canary_period():
    """Canary byte at arena offset p is f(p mod 2^16): an odd multiple of the low
    byte (a permutation of 0..255 within each page, neighbours differ by 167)
    plus a per-page term, so pages differ too."""
    p = np.arange(_PERIOD, dtype=np.int64)
    return (((p & 0xFF) * 167 + (p >> 8) * 29 + 0x5A) & 0xFF).astype(np.uint8)


class Carve:
    def __init__(self, name, off, nbytes, cap, lo, hi):
        self.name, self.off, self.nbytes = name, off, nbytes
        self.cap = cap          # bytes reserved (>= nbytes; a reused carve may use fewer)
        self.lo, self.hi = lo, hi  # strip starts at lo, the trailing strip ends at hi

    def __repr__(self):
        return "Carve(%s, off=%d, nbytes=%d)" % (self.name, self.off, self.nbytes)


class ZeroWorkspace:
    """What a wrapper gets when it asks for a 0-byte workspace: a pointer into
    canary and length 0 (an empty torch view reports a null data_ptr)."""

    def __init__(self, ptr, device):
        self._ptr, self.device = ptr, device

    def data_ptr(self):
        return self._ptr

    def numel(self):
        return 0


class Arena:
    """One uint8 allocation filled with canary; carve() hands out exact views."""

    def __init__(self, device, nbytes=32 << 20):
        self.device = torch.device(device)
        self.nbytes = _round_up(nbytes, _PERIOD)
        self.buf = torch.empty(self.nbytes, dtype=torch.uint8, device=self.device)
        self._period = torch.from_numpy(_canary_period()).to(self.device)
        self.reset()

    # -- layout ----------------------------------------------------------------
    def reset(self):
        """Forget every carve and repaint the whole arena with canary."""
        self.buf.view(-1, _PERIOD)[:] = self._period
        self.carves = []
        self._by_key = {}
        self._top = 0
        self._tail = 0

    def _expected(self, a, b):
        """Canary bytes of arena offsets [a, b)."""
        idx = torch.arange(a, b, device=self.device, dtype=torch.int64) & (_PERIOD - 1)
        return self._period[idx]

    def _paint(self, a, b):
        if b > a:
            self.buf[a:b] = self._expected(a, b)

    def carve(self, shape, dtype=torch.uint8, fill=ZERO, name=None, strip=0, key=None):
        """A contiguous `dtype` view of `shape` with exactly its own bytes.

        fill: ZERO / ONES / any byte value written over the view, or KEEP.
        strip: extra lower bound for the canary strips in bytes (a workspace's slot
          size); the leading-dimension stride of `shape` is applied by itself.
        key: carves with the same key share one offset ("reuse" mode): a later
          request of at most the first one's size gets the same offset, keeps the
          bytes it covers unless `fill` says otherwise, and the bytes of the
          earlier, larger carve beyond it are repainted as canary so the trailing
          strip is again adjacent.
        """
        shape = (int(shape),) if isinstance(shape, (int, np.integer)) else tuple(int(s) for s in shape)
        item = torch.empty((), dtype=dtype).element_size()
        nbytes = int(np.prod(shape, dtype=np.int64)) * item if len(shape) else item
        row = (nbytes // shape[0]) if len(shape) and shape[0] > 0 else 0
        guard = _round_up(max(MIN_STRIP, row, int(strip)))
        name = name or "carve%d" % len(self.carves)
        c = self._by_key.get(key) if key is not None else None
        if c is not None and nbytes <= c.cap and guard <= c.off - c.lo:
            self._paint(c.off + nbytes, c.off + c.cap)
            c.nbytes = nbytes
            c.name = name
        else:
            # the strip between two carves serves both: the wider guard wins
            off = self._top + max(guard, self._tail)
            cap = max(_round_up(nbytes), ALIGN)  # a 0-byte carve still owns 256 bytes of canary
            hi = off + cap + guard
            if hi > self.nbytes:
                raise MemoryError("arena of %d bytes is full (carve %s wants %d + 2 * %d)"
                                  % (self.nbytes, name, nbytes, guard))
            # the bytes between nbytes and the 256-byte boundary stay canary: exact size
            c = Carve(name, off, nbytes, cap, self._top, hi)
            self.carves.append(c)
            if key is not None:
                self._by_key[key] = c
            self._top = off + cap
            self._tail = guard
        flat = self.buf[c.off:c.off + nbytes]
        if fill is not KEEP and nbytes:
            flat.fill_(int(fill))
        view = flat.view(dtype).view(shape) if nbytes else flat.view(dtype).reshape(shape)
        return view

    def ptr(self, carve_index=-1):
        return self.buf.data_ptr() + self.carves[carve_index].off

    # -- the check -------------------------------------------------------------
    def check(self, what=""):
        """Every canary byte is intact; otherwise name the carve whose strip was hit,
        with the first and last damaged offset relative to that carve and the count."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        end = self._top + self._tail  # carve() keeps this inside the arena
        if end == 0:
            return
        end = _round_up(end, _PERIOD)  # whole periods; past the last strip all is canary too
        bad = (self.buf[:end].view(-1, _PERIOD) != self._period).view(-1)
        for c in self.carves:
            bad[c.off:c.off + c.nbytes] = False
        if not bool(bad.any()):
            return
        pos = torch.nonzero(bad).flatten().cpu().numpy()
        lines = []
        for i, c in enumerate(self.carves):  # in offset order; a shared strip is split in half
            stop = c.off + c.nbytes
            lo = 0 if i == 0 else (self.carves[i - 1].off + self.carves[i - 1].nbytes + c.off) // 2
            hi = end if i + 1 == len(self.carves) else (stop + self.carves[i + 1].off) // 2
            before = pos[(pos >= lo) & (pos < c.off)]
            after = pos[(pos >= stop) & (pos < hi)]
            if len(before):
                lines.append("%s: %d canary bytes BEFORE it damaged, offsets %d..%d relative to "
                             "its start" % (c.name, len(before), before[0] - c.off,
                                            before[-1] - c.off))
            if len(after):
                lines.append("%s: %d canary bytes AFTER it damaged, offsets +%d..+%d past its "
                             "end (its size: %d bytes)" % (c.name, len(after), after[0] - stop,
                                                           after[-1] - stop, c.nbytes))
        if not lines:
            lines.append("%d canary bytes damaged at arena offsets %d..%d"
                         % (len(pos), pos[0], pos[-1]))
        raise AssertionError("canary damaged%s:\n  %s" % (" (" + what + ")" if what else "",
                                                          "\n  ".join(lines)))


def prefilled(view, fill):
    """True where the bytes of `view` still hold the prefill byte."""
    return view.contiguous().view(torch.uint8) == int(fill)


def assert_prefill(view, fill, what):
    """Untouched remainder: every byte of `view` is still the prefill byte."""
    if view.numel() == 0:
        return
    ok = prefilled(view, fill)
    if not bool(ok.all()):
        bad = torch.nonzero(~ok.flatten()).flatten()
        raise AssertionError("%s: %d bytes past the defined region were written (prefill 0x%02X), "
                             "first at byte %d, last at byte %d"
                             % (what, bad.numel(), int(fill), int(bad[0]), int(bad[-1])))


def guarded_ws(monkeypatch, arena, fill, reuse=False, strip=0):
    """Replace vosdetectron_amd.ops._ws: every workspace a wrapper asks for is
    carved at exactly `nbytes` bytes, pre-filled with `fill`.  A 0-byte request
    gets a pointer into 256 bytes of canary and length 0 (the 256-byte minimum of
    the real _ws is not reproduced).  reuse=True: successive requests of the same
    call site get the same offset without a refill.  strip: the workspace's
    slot size in bytes, or a function of the request's size that gives it (the canary
    strips are at least that wide).  Returns the list of (call site, nbytes, arena
    offset) requests made, for the test to assert on."""
    from vosdetectron_amd import ops
    log = []

    def _ws(nbytes, device):
        f = sys._getframe(1)
        site = "%s:%d" % (f.f_code.co_name, f.f_lineno)
        nbytes = int(nbytes)
        name = "workspace of %s (%d bytes)" % (site, nbytes)
        key = ("ws", site) if reuse else None
        known = reuse and key in arena._by_key and nbytes <= arena._by_key[key].cap
        v = arena.carve((nbytes,), torch.uint8, KEEP if known else fill, name=name,
                        strip=strip(nbytes) if callable(strip) else strip, key=key)
        c = arena._by_key[key] if reuse else arena.carves[-1]
        log.append((site, nbytes, c.off))
        if nbytes == 0:
            return ZeroWorkspace(arena.buf.data_ptr() + c.off, arena.device)
        return v

    monkeypatch.setattr(ops, "_ws", _ws)
    return log


class _TorchProxy:
    """`torch` as vosdetectron_amd.ops sees it under guarded_alloc: every device tensor
    a wrapper allocates for itself (torch.empty / empty_like / zeros) is a carve."""

    def __init__(self, arena, fill, log):
        self._arena, self._fill, self._log = arena, fill, log

    def __getattr__(self, name):
        return getattr(torch, name)

    def _carve(self, shape, dtype, fill, memory_format):
        shape = tuple(int(s) for s in shape)
        name = "%s's own tensor %d %s" % (sys._getframe(2).f_code.co_name, len(self._log), shape)
        if memory_format is torch.channels_last and len(shape) == 4:
            B, C, H, W = shape
            v = self._arena.carve((B, H, W, C), dtype, fill, name).permute(0, 3, 1, 2)
        else:
            v = self._arena.carve(shape, dtype, fill, name)
        self._log.append(v)
        return v

    def _mine(self, device):
        return device is not None and torch.device(device).type == self._arena.device.type

    def empty(self, *shape, dtype=torch.float32, device=None, memory_format=None):
        if len(shape) == 1 and not isinstance(shape[0], int):
            shape = tuple(shape[0])
        if not self._mine(device):
            return torch.empty(shape, dtype=dtype, device=device)
        return self._carve(shape, dtype, self._fill, memory_format)

    def zeros(self, *shape, dtype=torch.float32, device=None):
        if len(shape) == 1 and not isinstance(shape[0], int):
            shape = tuple(shape[0])
        if not self._mine(device):
            return torch.zeros(shape, dtype=dtype, device=device)
        return self._carve(shape, dtype, ZERO, None)

    def empty_like(self, t, memory_format=None):
        cl = t.dim() == 4 and not t.is_contiguous() and \
            t.is_contiguous(memory_format=torch.channels_last)
        return self._carve(t.shape, t.dtype, self._fill, torch.channels_last if cl else None)


def guarded_alloc(monkeypatch, arena, fill):
    """For the wrappers that allocate their outputs inside: replace the `torch` name in
    vosdetectron_amd.ops so that every tensor the wrapper allocates on the arena's device
    is a carve pre-filled with `fill` (torch.zeros stays zeros: the wrapper relies on
    it).  The wrapper then passes the C entry its own argument list with pointers into
    carves.  Returns the list of the carved views, in allocation order."""
    from vosdetectron_amd import ops
    log = []
    monkeypatch.setattr(ops, "torch", _TorchProxy(arena, fill, log))
    return log


# --------------------------------------------------------------------------- shared by the GPU tests
WS_MODES = (ZERO, ONES, "leftover")


def to_dev(a, device="cuda"):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def to_np(t):
    return t.cpu().numpy()


def stream():
    return torch.cuda.current_stream().cuda_stream


def sweep(arena, small, large, verify):
    """small(ws_fill, out_fill) -> result, verified under every fill combination
    (workspace 0x00 / 0xFF / the leftover of large(...) run first in the same carves,
    times outputs 0x00 / 0xFF), the canaries checked after every call."""
    for out_fill in FILLS:
        for ws in WS_MODES:
            arena.reset()
            tag = "workspace %s, outputs 0x%02X" % (ws if ws == "leftover" else "0x%02X" % ws,
                                                    out_fill)
            if ws == "leftover":
                large(ONES, out_fill)
                arena.check("the larger instance before: " + tag)
                res = small(KEEP, out_fill)
            else:
                res = small(ws, out_fill)
            arena.check(tag)
            verify(res, out_fill, tag)


def rows_equal(got, want, what):
    """Bit for bit (the float32 words are compared as int32: NaN prefill never equals)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape,
                                                                 got.dtype, want.dtype)
    a = got.view(np.int32) if got.dtype == np.float32 else got
    b = want.view(np.int32) if want.dtype == np.float32 else want
    assert np.array_equal(a, b), "%s: %d of %d values differ" % (what, int((a != b).sum()), a.size)
