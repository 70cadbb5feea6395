"""Device tensors past 2^31 and 2^32 bytes for the GPU tier, checked without copying them to the host.

A tensor is `count` units (images, or blocks of rows) of `unit` bytes each, the last one cut to what the span leaves.
Unit i holds pattern[i % P] -- P distinct random units, P odd, so that an access off by 2^31 or 2^32 bytes lands on
another phase of the pattern -- except at the marker units, which hold units of their own. The oracle runs on the P
pattern units and the markers only; the expected output of unit i is that of its pattern unit or marker.

Both ends of every tensor carry GUARD bytes of a per-position pattern (_gpu.guard_pattern); comparisons run on the device
in chunks of at most CHUNK bytes, so that no temporary comes near the size of the tensors.
"""
import gc

import numpy as np

from _gpu import guard_pattern

GiB = 1 << 30
GUARD = 4096
CHUNK = 256 << 20
PERIOD = 7                  # odd: 2^31 and 2^32 are never a whole number of periods
BUDGET = 16 * GiB           # the most device memory one case may hold at its peak
BOUNDS = ((1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32)


def free_memory():
    import torch
    gc.collect()
    torch.cuda.empty_cache()


def require_memory(nbytes: int, what: str) -> None:
    """Fail -- never skip -- when the device cannot hold the case"""
    import torch
    assert nbytes <= BUDGET, f"{what}: {nbytes / GiB:.2f} GiB is over the {BUDGET / GiB:.0f} GiB budget of one case"
    free, total = torch.cuda.mem_get_info()
    assert free >= nbytes + CHUNK, (f"{what}: needs {(nbytes + CHUNK) / GiB:.2f} GiB of device memory, "
                                    f"{free / GiB:.2f} of {total / GiB:.2f} GiB free")


def markers(count: int, spans_units) -> list:
    """Indices of the units that hold bytes 2^31 - 1, 2^31, 2^32 - 1 and 2^32 of each (span, unit) tensor, and the last"""
    out = {count - 1}
    for span, unit in spans_units:
        out.update(b // unit for b in BOUNDS if b < span)
    return sorted(out)


class Tensor:
    """`span` bytes of device memory between two guards; `view` is the tensor"""

    def __init__(self, span: int, salt: int):
        import torch
        self.span = span
        self.buf = torch.empty(GUARD + span + GUARD, dtype=torch.uint8, device="cuda")
        self.view = self.buf[GUARD:GUARD + span]
        self.guards = torch.from_numpy(guard_pattern(2 * GUARD, salt)).cuda()
        self.buf[:GUARD].copy_(self.guards[:GUARD])
        self.buf[GUARD + span:].copy_(self.guards[GUARD:])

    def fill(self, value: int) -> None:
        self.view.fill_(value)

    def fill_units(self, unit: int, pattern: np.ndarray, marks: dict) -> None:
        """unit i = pattern[i % P], marks[i] where given (each cut to the span)"""
        import torch
        pat = torch.from_numpy(np.ascontiguousarray(pattern).reshape(-1)).cuda()
        period = pat.numel()
        whole = self.span // period
        if whole:
            self.view[:whole * period].view(whole, period).copy_(pat.view(1, period).expand(whole, period))
        rest = self.span - whole * period
        if rest:
            self.view[whole * period:].copy_(pat[:rest])
        for i, m in marks.items():
            lo = i * unit
            hi = min(lo + unit, self.span)
            self.view[lo:hi].copy_(torch.from_numpy(np.ascontiguousarray(m[:hi - lo])).cuda())

    def assert_guards(self, what: str) -> None:
        import torch
        torch.cuda.synchronize()
        for part, ref, where in ((self.buf[:GUARD], self.guards[:GUARD], "before"),
                                 (self.buf[GUARD + self.span:], self.guards[GUARD:], "after")):
            bad = (part != ref).nonzero()
            assert bad.numel() == 0, f"{what}: the guard {where} the tensor was written (byte {int(bad[0])} of it)"

    def assert_all(self, value: int, what: str) -> None:
        for lo in range(0, self.span, CHUNK):
            bad = (self.view[lo:lo + CHUNK] != value).nonzero()
            assert bad.numel() == 0, f"{what}: byte {lo + int(bad[0])} of {self.span} is not {value:#x}"
        self.assert_guards(what)

    def assert_units(self, unit: int, pattern: np.ndarray, marks: dict, what: str) -> None:
        """every unit equals its pattern unit or its marker, byte for byte; the guards are intact"""
        import torch
        P = pattern.shape[0]
        pat = torch.from_numpy(np.ascontiguousarray(pattern).reshape(-1)).cuda()
        period = P * unit
        whole = self.span // period
        step = max(1, CHUNK // period)
        for s in range(0, whole, step):
            e = min(whole, s + step)
            got = self.view[s * period:e * period].view(e - s, P, unit)
            bad = (got != pat.view(1, P, unit)).any(dim=2).view(-1).nonzero().view(-1)
            if bad.numel():
                wrong = [s * P + int(u) for u in bad.tolist() if s * P + int(u) not in marks]
                assert not wrong, self._where(what, unit, wrong[0], pat[(wrong[0] % P) * unit:(wrong[0] % P + 1) * unit])
        for u in range(whole * P, (self.span + unit - 1) // unit):
            if u in marks:
                continue
            lo, hi = u * unit, min((u + 1) * unit, self.span)
            want = pat[(u % P) * unit:(u % P) * unit + hi - lo]
            assert torch.equal(self.view[lo:hi], want), self._where(what, unit, u, want)
        for u, m in marks.items():
            lo, hi = u * unit, min((u + 1) * unit, self.span)
            want = torch.from_numpy(np.ascontiguousarray(m[:hi - lo])).cuda()
            assert torch.equal(self.view[lo:hi], want), self._where(what, unit, u, want, "marker ")
        self.assert_guards(what)

    def _where(self, what, unit, u, want, kind=""):
        lo = u * unit
        got = self.view[lo:lo + want.numel()]
        i = int((got != want).nonzero()[0])
        return (f"{what}: {kind}unit {u} of {(self.span + unit - 1) // unit} differs first at byte {lo + i} "
                f"({(lo + i) / GiB:.4f} GiB): got {int(got[i])}, want {int(want[i])}")


class SparseRows(Tensor):
    """`rows` rows of `channels` bytes, `stride` bytes apart, in a tensor too large to fill: only the rows and `near` bytes
    on either side of each are ever written or compared, the bytes between them are never touched"""

    def __init__(self, rows: int, stride: int, channels: int, salt: int, near: int = 4096):
        super().__init__((rows - 1) * stride + channels, salt)
        self.rows, self.stride, self.channels, self.near = rows, stride, channels, near

    def window(self, r: int):
        return max(r * self.stride - self.near, 0), min(r * self.stride + self.channels + self.near, self.span)

    def _expected(self, r: int, data, background: int) -> np.ndarray:
        lo, hi = self.window(r)
        want = np.full(hi - lo, background, np.uint8)
        if data is not None:
            want[r * self.stride - lo:r * self.stride - lo + self.channels] = data[r]
        return want

    def write(self, data, background: int) -> None:
        """every window = `background`, with row r = data[r] where data ([rows, channels]) is given"""
        import torch
        for r in range(self.rows):
            lo, hi = self.window(r)
            self.view[lo:hi].copy_(torch.from_numpy(self._expected(r, data, background)).cuda())

    def assert_rows(self, data, background: int, what: str) -> None:
        for r in range(self.rows):
            lo, hi = self.window(r)
            got, want = self.view[lo:hi].cpu().numpy(), self._expected(r, data, background)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (f"{what}: row {r} and its neighbourhood differ in {bad.size} bytes, first at byte {lo + int(bad[0])} "
                                   f"({(lo + int(bad[0])) / GiB:.4f} GiB): got {int(got[bad[0]])}, want {int(want[bad[0]])}")
        self.assert_guards(what)


def units(flat: np.ndarray, unit: int, n: int, fill: int) -> np.ndarray:
    """a tensor of n units whose last one is cut, as (n, unit) with the cut part `fill`"""
    out = np.full(n * unit, fill, np.uint8)
    out[:flat.size] = flat
    return out.reshape(n, unit)
