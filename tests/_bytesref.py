"""Host reference of the ByteImages norm table and the test images of the uint8 route.

table(mean, std) restates vqa_u8_norm_table with torch on the CPU: ((arange(256).float() / 255 - m) / s).to(bfloat16) per channel --
float32 true divisions in ToTensor / Normalize's order, then round-to-nearest-even to bf16.  tests/test_byte_images_cpu.py pins it
(monotone, the bf16 rounding of the fp32 value); the GPU tests compare the device table against it."""
import struct

import torch

IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
ODD = ((0.1, 0.73, -0.25), (0.05, 1.7, 0.31))             # one odd (mean, std): a negative mean, a std above 1


def table_f32(mean, std) -> torch.Tensor:
    v = torch.arange(256).float() / 255
    return torch.stack([(v - m) / s for m, s in zip(mean, std)])


def table(mean, std) -> torch.Tensor:
    return table_f32(mean, std).to(torch.bfloat16)


def f2bf_bits(x: float) -> int:
    """bf16 bits of an fp32 value, round to nearest even, by integer arithmetic on the fp32 bits."""
    u = struct.unpack("<I", struct.pack("<f", x))[0]
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF


def images(B: int, H: int, W: int, seed: int = 0) -> torch.Tensor:
    """uint8 [B, H, W, 3] (CPU): random bytes; the first and last rows and columns are 0 except the four corner pixels, which are 0
    (top left, bottom right) and 255 (top right, bottom left) -- a kernel that pads with table[0] or reads a byte past a row cannot
    reproduce the float route on it; image 0 holds every byte value in every channel (the batch does, where one image is too small)."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + 3 * H + W)
    x = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
    inner = (H - 2) * (W - 2)
    assert B * inner >= 256
    for c in range(3):                                     # every byte value: in image 0 alone when it has the room, else over the batch
        n = 1 if inner >= 256 else B
        flat = x[:n, 1:-1, 1:-1, c].reshape(-1).clone()
        flat[torch.randperm(n * inner, generator=g)[:256]] = torch.arange(256).to(torch.uint8)
        x[:n, 1:-1, 1:-1, c] = flat.view(n, H - 2, W - 2)
    x[:, 0], x[:, -1], x[:, :, 0], x[:, :, -1] = 0, 0, 0, 0
    x[:, 0, -1], x[:, -1, 0] = 255, 255
    return x
