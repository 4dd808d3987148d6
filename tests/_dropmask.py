"""numpy restatement of the dropout generator of the HIP kernels (csrc/common.h: mix32 / drop_key / drop_keep32), shared by the
dropout contract tests (test_gpu_dropout.py) and the in-situ checks of a live step (test_gpu_insitu.py)."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)


def _mix32(x):
    x = x & M32
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x7feb352d)) & M32
    x ^= x >> np.uint64(15); x = (x * np.uint64(0x846ca68b)) & M32
    x ^= x >> np.uint64(16)
    return x


def keep_mask(seed: int, n: int, p: float) -> np.ndarray:
    """numpy restatement of drop_keep32(drop_key(seed), idx, p) for idx in [0, n)."""
    key = (_mix32(np.uint64(seed & 0xFFFFFFFF)) ^ ((np.uint64(seed >> 32) * np.uint64(0x9E3779B9)) & M32)) & M32
    h = _mix32(np.arange(n, dtype=np.uint64) ^ key)
    u = (h >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return u >= np.float32(p)
