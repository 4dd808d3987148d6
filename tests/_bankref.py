"""Host reference of vqa_bank_batch: a batch drawn from a uint8 image bank by plain torch indexing on the CPU.  Nothing of the package
is used; tests/test_image_bank_cpu.py pins it against a literal triple loop and against oracle/input_oracle.py's resize -> crop -> flip."""
import torch


def bank_batch_ref(bank_cpu, rows, crop_yx, flip, O):
    """out[b][y][x][c] = bank[rows[b]][cy_b + y][cx_b + (flip_b ? O-1-x : x)][c].
    bank_cpu uint8 [n, S, S, 3]; rows [B]; crop_yx [B][2] as (y, x) or None (origin (0, 0)); flip [B] or None (no flip)."""
    rows = torch.as_tensor(rows, dtype=torch.long).reshape(-1)
    B = rows.shape[0]
    crop = torch.zeros(B, 2, dtype=torch.long) if crop_yx is None else torch.as_tensor(crop_yx, dtype=torch.long).reshape(B, 2)
    fl = torch.zeros(B, dtype=torch.bool) if flip is None else torch.as_tensor(flip).reshape(B).to(torch.bool)
    ar = torch.arange(O)
    ys = crop[:, 0, None] + ar[None, :]                                             # [B, O]
    xs = crop[:, 1, None] + torch.where(fl[:, None], O - 1 - ar[None, :], ar[None, :])  # [B, O]
    return bank_cpu[rows[:, None, None], ys[:, :, None], xs[:, None, :]].contiguous()   # [B, O, O, 3]
