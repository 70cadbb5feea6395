"""Device-memory plumbing for the GPU tier (torch is used for allocation/copies only)."""
import numpy as np


def to_device(arr: np.ndarray, misalign: int = 0):
    import torch
    arr = np.ascontiguousarray(arr)
    if misalign:
        t = torch.empty(arr.size + misalign, dtype=torch.uint8, device="cuda")
        view = t[misalign:]
        view.copy_(torch.from_numpy(arr.view(np.uint8).reshape(-1)))
        return view
    return torch.from_numpy(arr.view(np.uint8).reshape(-1).copy()).cuda()


def from_device(t) -> np.ndarray:
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().copy()


GUARD = 256   # bytes of known pattern on each side of a guarded buffer


def guard_pattern(n: int, salt: int) -> np.ndarray:
    """A per-position byte pattern (never a constant run, so a write shifted by any amount changes some byte)."""
    i = np.arange(n, dtype=np.uint32)
    return ((i * 131 + salt * 29 + (i >> 8) * 7 + 0x3C) & 0xFF).astype(np.uint8)


class Guarded:
    """`arr` in device memory at byte `offset` of a fresh allocation, between two guards of GUARD bytes or more:
    [guard | offset pad | data | guard]. `view` is the data; `intact()` says whether nothing outside it was written."""

    def __init__(self, arr: np.ndarray, offset: int = 0, guard: int = GUARD):
        import torch
        assert guard >= GUARD and offset >= 0
        data = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        self.offset, self.guard, self.n = offset, guard, data.size
        # torch's caching allocator hands out 512-byte aligned blocks: the guard keeps that, the offset moves the data
        assert guard % 16 == 0
        total = guard + offset + self.n + guard
        self.host = guard_pattern(total, offset)
        self.host[guard + offset:guard + offset + self.n] = data
        self.buf = torch.from_numpy(self.host.copy()).cuda()
        self.view = self.buf[guard + offset:guard + offset + self.n]
        assert self.view.data_ptr() % 16 == offset % 16, (hex(self.view.data_ptr()), offset)

    def data_ptr(self) -> int:
        return self.view.data_ptr()

    def read(self) -> np.ndarray:
        import torch
        torch.cuda.synchronize()
        return self.buf.cpu().numpy()[self.guard + self.offset:self.guard + self.offset + self.n].copy()

    def outside(self):
        """(index relative to the data start, got, want) of the first byte written outside the data, or None"""
        whole = self.buf.cpu().numpy()
        lo, hi = self.guard + self.offset, self.guard + self.offset + self.n
        for part, base in ((slice(0, lo), 0), (slice(hi, None), hi)):
            bad = np.flatnonzero(whole[part] != self.host[part])
            if bad.size:
                i = base + int(bad[0])
                return i - lo, int(whole[i]), int(self.host[i])
        return None

    def assert_intact(self, what: str) -> None:
        import torch
        torch.cuda.synchronize()
        hit = self.outside()
        assert hit is None, (f"{what}: byte {hit[0]} relative to the data start ({self.n} bytes) was written: "
                             f"{hit[1]}, guard pattern {hit[2]}")
