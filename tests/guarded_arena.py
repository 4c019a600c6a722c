"""A guard-band arena for the device-pointer (_async) entry points of the C ABI.

Every buffer of one call -- inputs, LUTs, index arrays, output, scratch -- is a region of ONE torch.uint8
tensor, with a guard band before the first region, between any two and after the last.  Guards and
writable regions hold a position-dependent pseudo-random stream (splitmix64 of the 8-byte word index,
seeded per fill), which neither a constant nor a copy from elsewhere reproduces; read-only regions hold
their data.  After the call, check() names every guard band and read-only region whose bytes changed.

Layout rules:
  - a band is at least twice the row size of the wider adjacent region and never under 64 KiB (a row
    is one ciphertext, GLWE or LUT: `row` of region(), the whole region when it is not given);
  - a region starts at an address that is `align` modulo 256 and no more aligned than that (align = 16:
    16-byte aligned, not 32), weaker than anything torch's allocators hand out, so a kernel that
    silently needs more than the header documents shows up.

Use: declare every region with region(), call allocate(), take the views with view(name) (region()
returns a handle whose .view is the same thing).  The arena proves that a call wrote nothing within a
guard's width of its buffers and changed no input; it sees reads only through what they do to the
output, and it is no sanitizer: a store further away than a guard band lands outside it unseen.
"""
import numpy as np
import torch

MIN_GUARD = 64 * 1024
_MASK64 = (1 << 64) - 1


def _i64(v: int) -> int:
    """the two's-complement int64 of a 64-bit pattern"""
    v &= _MASK64
    return v - (1 << 64) if v >> 63 else v


def _lsr(x, s: int):
    """logical right shift of an int64 tensor (torch's >> is arithmetic)"""
    return (x >> s) & ((1 << (64 - s)) - 1)


def splitmix64(first_word: int, nwords: int, seed: int, device) -> torch.Tensor:
    """words [first_word, first_word + nwords) of the stream of `seed`, as int64 bit patterns:
    splitmix64's output function on (seed + 1) * golden + index * golden"""
    idx = torch.arange(first_word, first_word + nwords, dtype=torch.int64, device=device)
    z = (idx + (seed + 1)) * _i64(0x9E3779B97F4A7C15)
    z = (z ^ _lsr(z, 30)) * _i64(0xBF58476D1CE4E5B9)
    z = (z ^ _lsr(z, 27)) * _i64(0x94D049BB133111EB)
    return z ^ _lsr(z, 31)


def splitmix64_int(index: int, seed: int) -> int:
    """the same word in plain Python integers (the helper's own test restates the stream with it)"""
    z = ((index + seed + 1) * 0x9E3779B97F4A7C15) & _MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
    return z ^ (z >> 31)


class Region:
    def __init__(self, name, nbytes, align, data, writable, row):
        self.name, self.nbytes, self.align, self.writable = name, int(nbytes), int(align), bool(writable)
        self.row = int(row) if row else int(nbytes)
        self.data = data
        self.offset = None  # byte offset in the arena, set by allocate()
        self.view = None    # the contiguous uint8 view, set by allocate()


def _as_bytes(data, nbytes: int) -> torch.Tensor:
    if isinstance(data, torch.Tensor):
        b = data.contiguous().view(torch.uint8).reshape(-1).cpu()
    else:
        b = torch.from_numpy(np.ascontiguousarray(data).view(np.uint8).reshape(-1).copy())
    if b.numel() != nbytes:
        raise ValueError(f"region data has {b.numel()} bytes, declared {nbytes}")
    return b


class GuardedArena:
    def __init__(self, device="cpu", seed: int = 1):
        self.device = torch.device(device)
        self.seed = seed
        self.regions = []
        self.segments = []  # (name, start, end, kind) over the whole arena, kind in guard / ro / rw
        self.buf = None

    # -- declaration ----------------------------------------------------------------------------
    def region(self, name, nbytes, align=16, data=None, writable=False, row=None) -> Region:
        """Declare a region of `nbytes` bytes starting at an address = align (mod 256).  `data`
        (numpy array or tensor of exactly nbytes bytes) is what a read-only region holds; a writable
        region holds the random stream unless data is given (an in-place operand).  `row`: bytes of
        one ciphertext / GLWE / LUT of the region, for the width of the bands next to it."""
        if self.buf is not None:
            raise RuntimeError("regions are declared before the arena is allocated")
        if align <= 0 or align >= 256 or align & (align - 1):
            raise ValueError("align must be a power of two below 256")
        if any(r.name == name for r in self.regions):
            raise ValueError(f"region {name} declared twice")
        if nbytes <= 0:
            raise ValueError("a region has at least one byte")
        if data is None and not writable:
            raise ValueError(f"read-only region {name} needs data")
        r = Region(name, nbytes, align, None if data is None else _as_bytes(data, nbytes), writable, row)
        self.regions.append(r)
        return r

    @staticmethod
    def band_bytes(row_a: int, row_b: int) -> int:
        return max(MIN_GUARD, 2 * max(row_a, row_b))

    def allocate(self) -> "GuardedArena":
        if self.buf is not None or not self.regions:
            raise RuntimeError("allocate() runs once, after at least one region()")
        pos, prev = 0, None
        for r in self.regions:
            band = self.band_bytes(prev.row if prev else 0, r.row)
            r.offset = (pos + band + 255) // 256 * 256 + r.align
            pos = r.offset + r.nbytes
            prev = r
        last = self.regions[-1]
        total = (pos + self.band_bytes(last.row, 0) + 7) // 8 * 8
        raw = torch.empty(total + 256, dtype=torch.uint8, device=self.device)
        skew = (-raw.data_ptr()) % 256  # torch's GPU blocks are 512-aligned, its CPU ones are not
        self._raw = raw
        self.buf = raw[skew:skew + total]
        assert self.buf.data_ptr() % 256 == 0
        pos = 0
        for i, r in enumerate(self.regions):
            left = self.regions[i - 1].name if i else ""
            self.segments.append((f"guard[{left}|{r.name}]", pos, r.offset, "guard"))
            self.segments.append((r.name, r.offset, r.offset + r.nbytes, "rw" if r.writable else "ro"))
            pos = r.offset + r.nbytes
            r.view = self.buf[r.offset:r.offset + r.nbytes]
            assert r.view.is_contiguous() and r.view.data_ptr() % 256 == r.align
        self.segments.append((f"guard[{last.name}|]", pos, total, "guard"))
        self._expect = torch.empty_like(self.buf)
        self._fill(self.seed, first=True)
        return self

    def view(self, name) -> torch.Tensor:
        for r in self.regions:
            if r.name == name:
                if r.view is None:
                    raise RuntimeError("allocate() the arena first")
                return r.view
        raise KeyError(name)

    # -- fill and check -------------------------------------------------------------------------
    def _fill(self, seed: int, first: bool) -> None:
        total = self.buf.numel()
        stream = splitmix64(0, total // 8, seed, self.device).view(torch.uint8)
        for name, a, b, kind in self.segments:
            if kind != "ro" or first:
                self.buf[a:b] = stream[a:b]
        if first:
            for r in self.regions:
                if r.data is not None:
                    r.view.copy_(r.data.to(self.device))
        self._expect.copy_(self.buf)
        self.seed = seed

    def refill(self, seed: int) -> None:
        """Rewrite the guards and the writable regions with the stream of another seed (read-only regions
        keep their data; a writable region loses the data it was declared with: restore it by hand)."""
        if seed == self.seed:
            raise ValueError("refill with a different seed")
        self._fill(seed, first=False)

    def restore(self) -> None:
        """Put back the data of the writable regions declared with data (in-place operands)."""
        for r in self.regions:
            if r.writable and r.data is not None:
                r.view.copy_(r.data.to(self.device))

    def check(self):
        """[(name, first, last)]: every guard band and read-only region with a changed byte, with the
        offsets (from the band's or region's start) of its first and last changed byte."""
        diff = self.buf != self._expect
        for name, a, b, kind in self.segments:
            if kind == "rw":
                diff[a:b] = False
        if not bool(diff.any()):
            return []
        out = []
        for name, a, b, kind in self.segments:
            if kind == "rw":
                continue
            nz = torch.nonzero(diff[a:b]).reshape(-1)
            if nz.numel():
                out.append((name, int(nz[0]), int(nz[-1])))
        return out
