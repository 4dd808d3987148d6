"""Operands inside NaN moats.  Importable without a GPU (device="cpu" serves tests/test_arena_cpu.py).

An Arena owns one allocation per operand, laid out as

    [ moat 64 KiB | skew 16 B | payload | moat 64 KiB ]

Every byte that is not payload holds the fill pattern: the 32-bit word 0x7FC17FC1 (a NaN read as fp32, two NaNs read as bf16) for float
and integer operands, the byte 0xFF for uint8 image / MXFP8 code operands (the test's own byte table maps 255 to NaN; E8M0 0xFF is
the NaN scale).  A kernel that reads one element past either end of an operand therefore multiplies a NaN into its sums, and one that
writes there changes a byte check() compares.  The allocation starts on a 512-byte boundary (torch's allocator), so the payload
starts 16 bytes past one: the least alignment layout.py (ALIGN = 8 bf16 elements) and include/vqa_hip.h promise.

    put(cpu_tensor, dtype)   an input: uploaded, its bits kept; check() wants them unchanged (the kernels take inputs const)
    out(shape, dtype)        an output documented as overwritten: payload prefilled with the pattern; check() wants none left
    acc(cpu_tensor)          a += output or caller-zeroed accumulator: prefilled with the given exact values; payload is free
    scratch(n)               n fp32 words of workspace, NaN-filled, exactly the size the matching query reports; payload is free
    check()                  every moat byte unchanged, inputs bit-identical, out() payloads fully overwritten

Failures name the operand, the side and the first offending byte offset."""
import torch

MOAT = 64 * 1024
SKEW = 16
FILL_WORD = 0x7FC17FC1
FILL_BYTE = 0xFF
BOUNDARY = 512

_INPUT, _OUT, _FREE = "input", "out", "free"


def fill_bytes(nbytes, byte_fill):
    """the fill pattern for a buffer of nbytes (a multiple of 4) as a CPU uint8 tensor"""
    if byte_fill:
        return torch.full((nbytes,), FILL_BYTE, dtype=torch.uint8)
    return torch.full((nbytes // 4,), FILL_WORD, dtype=torch.int32).view(torch.uint8).clone()


def bits(t):
    """the bytes of a contiguous CPU tensor"""
    return t.contiguous().view(-1).view(torch.uint8)


class Operand:
    def __init__(self, name, kind, buf, image, lo, nbytes, tensor):
        self.name, self.kind, self.buf, self.image = name, kind, buf, image       # image: the CPU bytes the buffer was given
        self.lo, self.nbytes, self.t = lo, nbytes, tensor
        self.may_stay = None

    def ptr(self):
        return self.t.data_ptr()


class Arena:
    def __init__(self, device="cuda"):
        self.device = device
        self.ops = []

    # ------------------------------------------------------------------------------------------ allocation
    def _place(self, name, kind, payload_bytes_cpu, shape, dtype, byte_fill, skew):
        nbytes = int(payload_bytes_cpu.numel())
        assert skew % 16 == 0 and 0 < skew < BOUNDARY or skew == 0
        lo = MOAT + skew
        total = (lo + nbytes + MOAT + 3) // 4 * 4
        image = fill_bytes(total, byte_fill)
        image[lo: lo + nbytes] = payload_bytes_cpu
        buf = image.to(self.device) if self.device != "cpu" else image.clone()
        assert buf.data_ptr() % BOUNDARY == 0 or self.device == "cpu", "the allocator no longer returns 512-byte aligned blocks"
        t = buf[lo: lo + nbytes].view(dtype).view(shape)
        op = Operand(name or f"operand{len(self.ops)}", kind, buf, image, lo, nbytes, t)
        self.ops.append(op)
        return op

    def put(self, cpu_tensor, dtype=None, name=None, byte_fill=None, skew=SKEW):
        """Upload an input.  Returns the device tensor (a view of the payload)."""
        src = cpu_tensor.detach().cpu()
        src = (src.to(dtype) if dtype is not None else src).contiguous()
        bf = (src.dtype == torch.uint8) if byte_fill is None else byte_fill
        return self._place(name, _INPUT, bits(src), src.shape, src.dtype, bf, skew).t

    def out(self, shape, dtype, name=None, byte_fill=None, skew=SKEW, may_stay=None):
        """An output the entry documents as overwritten.  may_stay: a CPU bool mask of `shape`, True where the case leaves an element
        legitimately untouched (e.g. rows past H - 1 a kernel never writes)."""
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        n = 1
        for s in shape:
            n *= s
        nbytes = n * torch.empty((), dtype=dtype).element_size()
        bf = (dtype == torch.uint8) if byte_fill is None else byte_fill
        # the payload follows the pattern of its absolute position, so 16-bit elements read 0x7FC1 whatever the parity of the offset
        pay = fill_bytes((MOAT + skew + nbytes + 3) // 4 * 4, bf)[MOAT + skew: MOAT + skew + nbytes]
        op = self._place(name, _OUT, pay, shape, dtype, bf, skew)
        op.may_stay = may_stay
        return op.t

    def acc(self, cpu_tensor, dtype=None, name=None, skew=SKEW):
        """A += output (weight gradient) or a caller-zeroed accumulator, prefilled with exact values."""
        src = cpu_tensor.detach().cpu()
        src = (src.to(dtype) if dtype is not None else src).contiguous()
        return self._place(name, _FREE, bits(src), src.shape, src.dtype, False, skew).t

    def scratch(self, nfloats, name=None, skew=SKEW):
        """fp32 workspace of exactly nfloats words, NaN-filled (entries must not rely on its contents)."""
        pay = fill_bytes(int(nfloats) * 4, False)
        return self._place(name, _FREE, pay, (int(nfloats),), torch.float32, False, skew).t

    # ------------------------------------------------------------------------------------------ the verdict
    @staticmethod
    def _first_diff(a, b):
        d = (a != b).nonzero()
        return None if d.numel() == 0 else int(d[0])

    def check(self):
        if self.device != "cpu":
            torch.cuda.synchronize()
        for op in self.ops:
            now = op.buf.cpu()
            lo, hi = op.lo, op.lo + op.nbytes
            i = self._first_diff(now[:lo], op.image[:lo])
            assert i is None, (f"{op.name}: low moat changed at byte {i - lo} relative to the payload start "
                               f"({int(now[i]):#04x}, was {int(op.image[i]):#04x})")
            i = self._first_diff(now[hi:], op.image[hi:])
            assert i is None, (f"{op.name}: high moat changed at byte {i} past the payload end "
                               f"({int(now[hi + i]):#04x}, was {int(op.image[hi + i]):#04x})")
            if op.kind == _INPUT:
                i = self._first_diff(now[lo:hi], op.image[lo:hi])
                assert i is None, f"{op.name}: input payload changed at byte {i} ({int(now[lo + i]):#04x}, was {int(op.image[lo + i]):#04x})"
            elif op.kind == _OUT:
                left = self.untouched(op, now)
                if op.may_stay is not None:
                    left = left & ~op.may_stay.reshape(-1)
                j = left.nonzero()
                assert j.numel() == 0, (f"{op.name}: out payload not overwritten: {int(left.sum())} of {left.numel()} elements still "
                                        f"hold the fill pattern, first at byte {int(j[0]) * op.t.element_size()}")

    @staticmethod
    def untouched(op, now):
        """per element of an out() payload: does it still hold the fill pattern (all its bytes)?"""
        es = op.t.element_size()
        same = (now[op.lo: op.lo + op.nbytes] == op.image[op.lo: op.lo + op.nbytes]).view(-1, es)
        return same.all(dim=1)

    def operand(self, tensor):
        for op in self.ops:
            if op.t is tensor:
                return op
        raise KeyError("not an operand of this arena")

