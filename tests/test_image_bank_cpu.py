"""CPU: the image bank's surface without a device -- the host reference tests/_bankref.py is pinned against a literal loop and against
oracle/input_oracle.py's resize -> crop -> flip; vqa_bank_batch is declared, exported by the library built for gfx950 and refuses bad
arguments with 1000 before any HIP call; BankSampler (host only) orders, shards and resumes epochs; ImageBank.batch takes its draws
in gpu_collate_fn's order from its distributions (host logic, no launch)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from _bankref import bank_batch_ref
from _pkg import REPO, pkg, sub
from oracle import input_oracle as IO


def _IB():
    return pkg().load_dropin_image_bank()


# ---------------------------------------------------------------------------------------------------------------- the reference
def test_bankref_equals_a_literal_triple_loop():
    g = torch.Generator().manual_seed(3)
    bank = torch.randint(0, 256, (3, 8, 8, 3), generator=g, dtype=torch.uint8)
    rows, crop, flip, O = [2, 0, 2, 1], [[4, 0], [0, 4], [1, 3], [2, 2]], [0, 1, 1, 0], 4
    want = torch.zeros(4, O, O, 3, dtype=torch.uint8)
    for b in range(4):
        for y in range(O):
            for x in range(O):
                want[b, y, x] = bank[rows[b], crop[b][0] + y, crop[b][1] + (O - 1 - x if flip[b] else x)]
    assert torch.equal(bank_batch_ref(bank, rows, crop, flip, O), want)
    assert torch.equal(bank_batch_ref(bank, rows, None, None, 8), bank[rows])              # NULL origins, NULL flips, O == S: a gather
    assert torch.equal(bank_batch_ref(bank, rows, None, flip, 4), bank_batch_ref(bank, rows, [[0, 0]] * 4, flip, 4))


def test_bankref_on_an_oracle_filled_bank_equals_the_oracle_resize_crop_flip():
    S, O = 40, 32
    srcs = [IO.pattern_image(h, w, seed, bits) for h, w, seed, bits in ((37, 50, 1, 5), (64, 23, 2, 8), (40, 40, 3, 8))]
    bank = torch.from_numpy(np.stack([IO.pil_resize_bilinear(im, S, S) for im in srcs]))
    rows, crop, flip = [2, 0, 1, 0], [(8, 8), (0, 0), (3, 5), (8, 1)], [1, 0, 1, 1]
    got = bank_batch_ref(bank, rows, crop, flip, O)
    for b, (r, (cy, cx), f) in enumerate(zip(rows, crop, flip)):
        x = IO.pil_resize_bilinear(srcs[r], S, S)[cy:cy + O, cx:cx + O]                     # Resize, then RandomCrop ...
        x = x[:, ::-1] if f else x                                                          # ... then RandomHorizontalFlip
        assert np.array_equal(got[b].numpy(), x), b


# ---------------------------------------------------------------------------------------------------------------- the C entry
def test_header_declares_and_library_exports_vqa_bank_batch():
    txt = open(os.path.join(REPO, "include", "vqa_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+vqa_bank_batch\s*\((.*?)\)\s*;", txt, flags=re.S)
    assert m, "include/vqa_hip.h does not declare vqa_bank_batch"
    L = sub("_lib")
    assert len([a for a in m.group(1).split(",") if a.strip()]) == len(L.SIGNATURES["vqa_bank_batch"]) == 11
    assert "bank_ops.hip" in sub("build").SOURCES
    import __graft_entry__ as G
    G.build()
    assert hasattr(L.lib(), "vqa_bank_batch")


def test_vqa_bank_batch_refuses_bad_arguments_before_any_hip_call():
    import __graft_entry__ as G
    G.build()
    f = sub("_lib").lib().vqa_bank_batch       # (bank, n_rows, S, rows, crop_yx, flip, out, B, O, err, stream)
    ok = [4096, 10, 40, 4096, None, None, 8192, 3, 32, None, None]
    bad = [(0, None), (3, None), (6, None),                     # NULL bank / rows / out with B > 0
           (1, 0), (1, -5), (7, -1),                            # n_rows < 1, B < 0
           (2, 0), (2, 3), (8, 0), (8, 3),                      # S < 4, O < 4
           (2, 38), (8, 30),                                    # S % 4, O % 4
           (8, 44),                                             # O > S
           (0, 4096 + 8), (6, 8192 + 4)]                        # misaligned bank / out
    for pos, val in bad:
        a = list(ok)
        a[pos] = val
        assert f(*a) == 1000, (pos, val)
    for pos, val in ((2, 0), (8, 6), (1, 0)):                   # the shape rules hold for an empty batch too
        a = list(ok)
        a[7], a[pos] = 0, val
        assert f(*a) == 1000, (pos, val)
    assert f(None, 10, 40, None, None, None, None, 0, 32, None, None) == 0      # B == 0 launches nothing


# ---------------------------------------------------------------------------------------------------------------- BankSampler
def _epoch(s):
    return [b.clone() for b in s]


def test_sampler_epoch_is_a_permutation_epochs_differ_and_a_seed_reproduces():
    S = _IB().BankSampler
    s = S(23, 5, shuffle=True, seed=11)
    e0 = _epoch(s)
    assert len(e0) == len(s) == 5 and [len(b) for b in e0] == [5, 5, 5, 5, 3]
    assert all(b.dtype == torch.int64 for b in e0)
    assert sorted(torch.cat(e0).tolist()) == list(range(23))
    assert torch.equal(torch.cat(e0), torch.randperm(23, generator=torch.Generator().manual_seed(11)))
    assert torch.equal(torch.cat(_epoch(s)), torch.cat(e0))                     # no set_epoch: the same epoch again
    s.set_epoch(1)
    e1 = _epoch(s)
    assert sorted(torch.cat(e1).tolist()) == list(range(23)) and not torch.equal(torch.cat(e1), torch.cat(e0))
    t = S(23, 5, shuffle=True, seed=11)
    t.set_epoch(1)
    assert torch.equal(torch.cat(_epoch(t)), torch.cat(e1))
    assert not torch.equal(torch.cat(_epoch(S(23, 5, shuffle=True, seed=12))), torch.cat(e0))
    assert torch.equal(torch.cat(_epoch(S(23, 5, shuffle=False))), torch.arange(23))


def test_sampler_ranks_are_disjoint_and_equally_long():
    S = _IB().BankSampler
    parts = [torch.cat(_epoch(S(23, 4, seed=5, rank=r, world=3))) for r in range(3)]
    assert [len(p) for p in parts] == [7, 7, 7]
    allv = torch.cat(parts).tolist()
    assert len(set(allv)) == 21 and set(allv) <= set(range(23))
    order = torch.randperm(23, generator=torch.Generator().manual_seed(5))
    for r in range(3):
        assert torch.equal(parts[r], order[:21][r::3])
    with pytest.raises(ValueError):
        S(23, 4, rank=3, world=3)


def test_sampler_drop_last_both_ways():
    S = _IB().BankSampler
    keep, drop = S(23, 5, drop_last=False, seed=1), S(23, 5, drop_last=True, seed=1)
    assert len(keep) == 5 and len(drop) == 4
    ek, ed = _epoch(keep), _epoch(drop)
    assert [len(b) for b in ek] == [5, 5, 5, 5, 3] and [len(b) for b in ed] == [5, 5, 5, 5]
    assert all(torch.equal(a, b) for a, b in zip(ek, ed))
    assert len(S(20, 5, drop_last=False)) == len(S(20, 5, drop_last=True)) == 4


def test_sampler_state_dict_round_trip_resumes_indices_and_draws():
    S = _IB().BankSampler

    def run(s, it=None, upto=None):
        out = []
        for k, idx in enumerate(it if it is not None else s):
            out.append((idx.clone(), torch.rand(len(idx), generator=s.generator), torch.randint(0, 9, (len(idx), 2), generator=s.generator)))
            if upto is not None and k + 1 == upto:
                break
        return out

    full = S(23, 5, seed=4, rank=1, world=2)
    full.set_epoch(3)
    want = run(full)
    assert len(want) == 3                                                       # 11 samples per rank, batches of 5
    a = S(23, 5, seed=4, rank=1, world=2)
    a.set_epoch(3)
    head = run(a, upto=2)                                                       # stopped after batch 2 ...
    state = a.state_dict()
    assert state["epoch"] == 3 and state["next_batch"] == 2
    b = S(23, 5, seed=4, rank=1, world=2)                                       # ... and resumed in a fresh sampler
    b.load_state_dict(state)
    got = head + run(b)
    assert len(got) == len(want)
    for x, y in zip(got, want):
        assert all(torch.equal(p, q) for p, q in zip(x, y))
    other = S(23, 5, seed=4, rank=0, world=2)                                   # the draws' generator depends on the rank and the epoch
    other.set_epoch(3)
    assert not torch.equal(run(other)[0][1], want[0][1])
    full.set_epoch(4)
    assert not torch.equal(run(full)[0][1], want[0][1])


def test_sampler_five_batches_resume_after_two():
    S = _IB().BankSampler
    want = _epoch(S(23, 5, seed=9))
    a = S(23, 5, seed=9)
    it = iter(a)
    next(it), next(it)
    b = S(23, 5, seed=9)
    b.load_state_dict(a.state_dict())
    rest = _epoch(b)
    assert len(rest) == 3 and all(torch.equal(x, y) for x, y in zip(rest, want[2:]))


# ---------------------------------------------------------------------------------------------------------------- the draws
class _RecordingResizer:
    """Stands where gpu_collate_fn expects a DeviceImageResizer: records the draws it is handed and takes the jitter's draw from the
    generator at the point the real one does (behind crop and flip, inside the jitter's call)."""

    def __init__(self, size, crop, jitter):
        self.size, self.out, self.jitter = size, crop or size, jitter

    def __call__(self, images, crop_yx=None, flip=None, generator=None, output="float"):
        self.crop_yx, self.flip = crop_yx, flip
        self.params = self.jitter.draw(len(images), generator) if self.jitter is not None else None
        return None


@pytest.mark.parametrize("crop,flip_p,jit", [(32, 0.5, True), (None, 0.5, True), (32, 0.0, True), (32, 0.5, False), (None, 0.0, False)])
def test_batch_draws_in_gpu_collate_order(crop, flip_p, jit):
    P, IB = pkg().load_dropin_preprocess(), _IB()
    jitter = P.DeviceColorJitter(0.2, 0.2, 0.2, 0.1) if jit else None
    B = 6
    items = [(torch.zeros(5, 7, 3, dtype=torch.uint8), torch.zeros(4, dtype=torch.long), torch.ones(4, dtype=torch.long), i) for i in range(B)]
    g1, g2 = torch.Generator().manual_seed(77), torch.Generator().manual_seed(77)
    rec = _RecordingResizer(40, crop, jitter)
    P.gpu_collate_fn(items, device="cpu", flip_p=flip_p, generator=g1, resizer=rec, output="bytes")
    bank = IB.ImageBank(4, size=40, device="cpu")
    flip, crop_yx, params = bank.draw(B, crop=crop, flip_p=flip_p, jitter=jitter, generator=g2)
    assert (flip is None) == (rec.flip is None) == (flip_p == 0.0)
    if flip is not None:
        assert torch.equal(flip, rec.flip)
    assert (crop_yx is None) == (rec.crop_yx is None) == (crop is None)
    if crop_yx is not None:
        assert crop_yx.tolist() == rec.crop_yx and 0 <= int(crop_yx.min()) and int(crop_yx.max()) <= 8
    assert (params is None) == (rec.params is None)
    if params is not None:
        assert torch.equal(params[0], rec.params[0]) and torch.equal(params[1], rec.params[1])
    assert torch.equal(g1.get_state(), g2.get_state())                          # and nothing else was taken from the generator


def test_bank_host_checks_need_no_device():
    IB = _IB()
    bank = IB.ImageBank(3, size=8, device="cpu")
    assert (bank.rows, bank.capacity, bank.nbytes, tuple(bank.tensor().shape)) == (0, 3, 3 * 8 * 8 * 3, (0, 8, 8, 3))
    x = torch.arange(2 * 8 * 8 * 3, dtype=torch.int64).remainder(251).to(torch.uint8).view(2, 8, 8, 3)
    assert bank.append_resized(x) == 0 and bank.rows == 2 and torch.equal(bank.tensor(), x)
    with pytest.raises(ValueError):
        bank.append_resized(x)                                                  # 2 + 2 > 3: nothing is written
    with pytest.raises(ValueError):
        bank.append([torch.zeros(5, 6, 3, dtype=torch.uint8)] * 2)
    assert bank.rows == 2 and torch.equal(bank.tensor(), x)
    for wrong in (x.float(), x[:, :4], x.permute(0, 3, 1, 2), x[0]):
        with pytest.raises(RuntimeError):
            bank.append_resized(wrong)
    for wrong in (torch.zeros(5, 6, 3), torch.zeros(3, 5, 6, dtype=torch.uint8), torch.zeros(5, 6, dtype=torch.uint8)):
        with pytest.raises(RuntimeError):
            bank.append([wrong])
    assert bank.rows == 2
    with pytest.raises(IndexError):
        bank.batch(torch.tensor([0, 2]))                                        # row 2 is not filled
    with pytest.raises(IndexError):
        bank.batch(torch.tensor([-1]))
    with pytest.raises(ValueError):
        bank.batch(torch.tensor([0]), crop=4, crop_yx=[[5, 0]])                 # origin outside [0, 4]
    with pytest.raises(RuntimeError, match="GPU only"):
        bank.batch(torch.tensor([0, 1]))                                        # there is no CPU path
    for size in (0, 6, 2):
        with pytest.raises(ValueError):
            IB.ImageBank(3, size=size, device="cpu")
    with pytest.raises(ValueError):
        bank.batch(torch.tensor([0]), crop=6)
    assert pkg().load_dropin_image_bank() is IB
