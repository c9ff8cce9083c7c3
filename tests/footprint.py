"""Guard-band arena: pins WHERE a kernel entry reads and writes (tests/test_gpu_footprint.py; own unit tests in tests/test_footprint.py).

Every buffer a test hands to a kernel is a view into ONE torch.empty(nbytes, uint8) -- the arena -- laid out as

    [outer guard >= 4 MiB] [guard][buf 0][guard] [guard][buf 1][guard] ... [outer guard >= 4 MiB]

with each inner guard at least 256 rows of its buffer's own row pitch and at least 64 KiB: a whole mis-addressed 256-row tile, a plane too
far or a pitch ignored still lands in memory the test owns, where it is REPORTED instead of corrupting another live tensor of torch's
allocator pool (silent) or leaving the allocation (a fault on a machine others share).

Three kinds of region are registered, all as strided byte patterns (start, width, stride, count) of the arena:
    guard    in front of / behind a buffer: nobody may write it, and its value may reach no output;
    hole     inside a buffer, same rule: the gap columns [N, ldo) of a pitched output, the space between planes, rows behind M;
    scratch  "readable, value irrelevant": the kernel's contract lets it load these bytes (attention's rows behind the last sequence,
             the pad rows of a skinny operand), they are filled like a guard but a kernel that owns them may also store there.

run_twice() is the protocol of every test: fill all three kinds with 0x00, launch, keep the owned outputs, check guards and holes; the same
with 0xFF (NaN in fp16 / bf16 / fp32 / fp64, -1 as an integer); then the owned outputs of the two runs must be BIT-identical.  Two patterns,
because a kernel that writes zeros (or NaNs) outside its extent would hide in a matching fill; bit-identity, because then nothing outside
the declared extent influences a result.  The caller compares the returned outputs with its fp64 reference, so the identity is not vacuous.

Limits of the method.  A LOAD outside the contract whose value reaches no output cannot be seen from outside the kernel: the suite bounds
stores and influence, not addresses touched.  To make the read contracts binding anyway, the tests give the attention and skinny operands
exactly the extent include/vtamiq_hip.h promises (everything behind is guard, still inside the arena) at the shapes that maximise the
over-read -- S % 128 == 1 for the 4-wave kernel's query rows, S % 64 == 1 for key tiles, S % 256 == 1 for the 8-wave kernel's blocks -- and a
reviewer checks the header sentence against the load addresses in the code.  No assembly is inspected.

The layout arithmetic and violations() work on a CPU arena as well (device="cpu").
"""

from collections import namedtuple

import torch

ALIGN = 256
OUTER_GUARD = 4 << 20
MIN_GUARD = 64 << 10
GUARD_ROWS = 256

# one touched guard / hole: buffer name, "before" | "after" | "hole:<name>", byte offset of the first changed byte (from the buffer's end for
# "after", from its start -- negative -- for "before", from its start for a hole), number of changed bytes, and the same place as text
Violation = namedtuple("Violation", "buffer side offset changed where")


class FootprintError(AssertionError):
    """violations: [Violation]; mismatch: {output index: bool tensor (CPU) of the elements whose bits differ between the two fills}."""

    def __init__(self, msg, violations=(), mismatch=None):
        super().__init__(msg)
        self.violations, self.mismatch = list(violations), dict(mismatch or {})


def _round_up(a, b):
    return (a + b - 1) // b * b


def guard_bytes(pitch_bytes):
    """Inner guard of a buffer whose rows are pitch_bytes apart."""
    return _round_up(max(GUARD_ROWS * pitch_bytes, MIN_GUARD), ALIGN)


def _numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


def arena_bytes(specs):
    """Size of an arena that holds carve(*spec) for every spec = (shape, dtype[, pitch_bytes]) in order (the alignment slack included)."""
    n = OUTER_GUARD + ALIGN
    for spec in specs:
        shape, dtype = spec[0], spec[1]
        isz = torch.empty((), dtype=dtype).element_size()
        pitch = spec[2] if len(spec) > 2 and spec[2] else (int(shape[-1]) if len(shape) else 1) * isz
        n += 2 * guard_bytes(pitch) + _round_up(_numel(shape) * isz, ALIGN)
    return n + OUTER_GUARD


class _Buf:
    def __init__(self, name, start, nbytes, isz, pitch, plane):
        self.name, self.start, self.nbytes, self.isz, self.pitch, self.plane = name, start, nbytes, isz, pitch, plane

    def where(self, off):
        """Byte offset from the buffer's start -> text; (plane, row, column) when the buffer has a pitch."""
        if not self.pitch:
            return f"byte {off}"
        pl, r = divmod(off, self.plane) if self.plane else (0, off)
        row, c = divmod(r, self.pitch)
        return f"plane {pl} row {row} column {c // self.isz}" if self.plane else f"row {row} column {c // self.isz}"


class _Region:
    def __init__(self, buf, kind, side, start, width, stride, count):
        self.buf, self.kind, self.side, self.start, self.width, self.stride, self.count = buf, kind, side, start, width, stride, count


class Arena:
    def __init__(self, nbytes, device="cpu"):
        self.mem = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        self.nbytes = int(nbytes)
        self._skew = (-self.mem.data_ptr()) % ALIGN             # so that carved views are 256-byte aligned in the address space
        self._cursor = OUTER_GUARD + self._skew                 # end of what has been laid out
        self.bufs, self.regions = {}, []
        self._tail = None                                       # the outer guard behind the last buffer (moves with every carve)

    # ---- layout ------------------------------------------------------------------------------------------------------
    def carve(self, name, shape, dtype, pitch_bytes=None, plane_bytes=None):
        """A view of `shape` / `dtype` with its own guards in front and behind.  pitch_bytes: the row pitch that sizes the guards and
        translates offsets (default: the last dimension); plane_bytes: distance of two planes, for the translation only."""
        assert name not in self.bufs, name
        isz = torch.empty((), dtype=dtype).element_size()
        shape = tuple(int(s) for s in shape)
        pitch = int(pitch_bytes) if pitch_bytes else (shape[-1] if shape else 1) * isz
        g = guard_bytes(pitch)
        nbytes = _numel(shape) * isz
        first = not self.bufs
        g_start = 0 if first else self._cursor                  # the first buffer's front guard is the outer guard (>= 4 MiB)
        start = self._cursor + g
        assert (self.mem.data_ptr() + start) % ALIGN == 0
        end = start + nbytes
        after = _round_up(end - self._skew + g, ALIGN) + self._skew
        if after + OUTER_GUARD > self.nbytes:
            raise ValueError(f"arena of {self.nbytes} bytes is too small for {name}: {after + OUTER_GUARD} needed")
        b = _Buf(name, start, nbytes, isz, pitch if len(shape) > 1 or pitch_bytes else 0, int(plane_bytes or 0))
        self.bufs[name] = b
        self.regions.append(_Region(b, "guard", "before", g_start, start - g_start, 0, 1))
        if self._tail is not None:                              # the previous last buffer: its rear guard ends where this one's guard begins
            self._tail.width = g_start - self._tail.start
        self._tail = _Region(b, "guard", "after", end, self.nbytes - end, 0, 1)
        self.regions.append(self._tail)
        self._cursor = after
        return self.mem[start:end].view(dtype).view(shape)

    def _add(self, kind, buf, name, start, width, stride=0, count=1):
        """Register bytes [start + i * stride, + width) for i < count, offsets from the start of buffer `buf`, as a hole or as scratch."""
        b = self.bufs[buf]
        if width <= 0 or count <= 0:
            return None
        last = start + (count - 1) * stride + width
        assert 0 <= start and (kind == "scratch" or last <= b.nbytes), (buf, name, start, width, stride, count)
        assert count == 1 or stride >= width
        r = _Region(b, kind, "hole:" + name, b.start + start, int(width), int(stride), int(count))
        assert r.start + (count - 1) * stride + width <= self.nbytes - OUTER_GUARD
        self.regions.append(r)
        return r

    def hole(self, buf, name, start, width, stride=0, count=1):
        """Bytes inside buffer `buf` that no kernel may write and whose value may reach no output."""
        return self._add("hole", buf, name, start, width, stride, count)

    def scratch(self, buf, name, start, width, stride=0, count=1):
        """Bytes of buffer `buf` the contract calls readable with an irrelevant value: filled with each pattern, not checked."""
        return self._add("scratch", buf, name, start, width, stride, count)

    # ---- patterns ----------------------------------------------------------------------------------------------------
    def _view(self, r):
        if r.count == 1:
            return self.mem[r.start:r.start + r.width]
        return self.mem.as_strided((r.count, r.width), (r.stride, 1), r.start)

    def fill(self, what, byte):
        """Fill a registered region, or a tensor that is a view of this arena, with `byte`."""
        if isinstance(what, _Region):
            self._view(what).fill_(byte)
        else:
            assert what.untyped_storage().data_ptr() == self.mem.untyped_storage().data_ptr(), "not a view of this arena"
            assert byte in (0x00, 0xFF)                         # through a same-size integer type: strided views work as well
            what.view({1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[what.element_size()]).fill_(-1 if byte else 0)

    def fill_guards(self, byte):
        """Every guard, hole and scratch region."""
        for r in self.regions:
            self._view(r).fill_(byte)

    def violations(self, byte):
        """One record per guard / hole that does not hold `byte` everywhere (compared on the arena's device)."""
        checked = [r for r in self.regions if r.kind != "scratch"]
        if not checked:
            return []
        counts = torch.stack([(self._view(r) != byte).sum() for r in checked]).cpu().tolist()
        out = []
        for r, n in zip(checked, counts):
            if not n:
                continue
            bad = (self._view(r) != byte).reshape(-1)
            i = int(torch.nonzero(bad)[0, 0])
            pos = r.start + (i // r.width) * r.stride + i % r.width if r.count > 1 else r.start + i
            b = r.buf
            off = pos - (b.start + b.nbytes) if r.side == "after" else pos - b.start
            out.append(Violation(b.name, r.side, off, int(n), b.where(pos - b.start) if pos >= b.start else f"{b.start - pos} bytes in front"))
        return out

    @staticmethod
    def describe(violations):
        return "; ".join(f"{v.buffer} [{v.side}] first changed byte at offset {v.offset} ({v.where}), {v.changed} bytes changed" for v in violations)

    # ---- the protocol ------------------------------------------------------------------------------------------------
    def run_twice(self, launch, outputs, prepare=None):
        """launch(): the call under test; outputs(): the OWNED outputs as a list of tensors (views without their holes); prepare(): restore
        what a launch consumes (an in-place residual stream; it runs before the fill, so it may write over holes).  Returns the outputs (copies) of the first run."""
        runs = []
        for byte in (0x00, 0xFF):
            if prepare is not None:
                prepare()
            self.fill_guards(byte)
            launch()
            if self.mem.is_cuda:
                torch.cuda.synchronize(self.mem.device)
            runs.append([o.clone(memory_format=torch.contiguous_format) for o in outputs()])
            v = self.violations(byte)
            if v:
                raise FootprintError(f"fill 0x{byte:02X}: written outside the contract: " + self.describe(v), violations=v)
        mismatch = {}
        for i, (a, b) in enumerate(zip(*runs)):
            ne = a.reshape(-1).view(torch.uint8) != b.reshape(-1).view(torch.uint8)
            if bool(ne.any()):
                mismatch[i] = ne.view(-1, a.element_size()).any(-1).view(a.shape).cpu()
        if mismatch:
            txt = "; ".join(f"output {i}: {int(m.sum())} of {m.numel()} elements, first at index {tuple(torch.nonzero(m)[0].tolist())}" for i, m in mismatch.items())
            raise FootprintError("outputs depend on bytes outside the declared extent (0x00 fill vs 0xFF fill): " + txt, mismatch=mismatch)
        return runs[0]
