"""GPU: the image bank -- vqa_bank_batch against tests/_bankref.py (torch.equal: bytes are copied), ImageBank's fill against the
existing resizer, the whole draw against the two existing routes of the training transform (DeviceImageResizer with crop / flip /
jitter, and gpu_collate_fn with one generator state) and against oracle/input_oracle.py, BankLoader's batches against direct gathers
of its table, and HipTrainer.step on a loader batch against the step on the same bytes in a hand-made ByteImages.
Kernel tests put the bank and the output in the interior of larger buffers filled with a sentinel byte: a stray read shows as wrong
bytes and a stray write as a damaged guard, never as a fault."""
import numpy as np
import pytest
import torch

import _bytesref as R
from _bankref import bank_batch_ref
from _pkg import pkg, sub
from oracle import input_oracle as IO
from oracle import vqa_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT, PAD = 0xA5, 4096                                   # guard byte and guard length (a multiple of 16: the interiors stay aligned)
N_BANK = 5
_CACHE = {}


def _IB():
    return pkg().load_dropin_image_bank()


def _P():
    return pkg().load_dropin_preprocess()


def _bank(S, seed=0):
    if ("bank", S, seed) not in _CACHE:
        g = torch.Generator().manual_seed(100 * S + seed)
        _CACHE[("bank", S, seed)] = torch.randint(0, 256, (N_BANK, S, S, 3), generator=g, dtype=torch.uint8)
    return _CACHE[("bank", S, seed)]


def _run(bank_cpu, rows, crop_yx, flip, O_, n_rows=None):
    """vqa_bank_batch between guards: returns (out uint8 [B, O, O, 3] on the CPU -- SENT where nothing was written --, err count)."""
    L = sub("_lib")
    n, S = bank_cpu.shape[:2]
    B = len(rows)
    big = torch.full((2 * PAD + bank_cpu.numel(),), SENT, dtype=torch.uint8, device=DEV)
    big[PAD: PAD + bank_cpu.numel()] = bank_cpu.reshape(-1).to(DEV)
    obig = torch.full((2 * PAD + B * O_ * O_ * 3,), SENT, dtype=torch.uint8, device=DEV)
    rows_d = torch.tensor(rows, dtype=torch.int32, device=DEV)
    crop_d = None if crop_yx is None else torch.tensor(crop_yx, dtype=torch.int32, device=DEV).reshape(B, 2).contiguous()
    flip_d = None if flip is None else torch.tensor(flip, dtype=torch.uint8, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    L.call("vqa_bank_batch", big.data_ptr() + PAD, n if n_rows is None else n_rows, S, rows_d.data_ptr(), L.ptr(crop_d), L.ptr(flip_d),
           obig.data_ptr() + PAD, B, O_, err.data_ptr())
    torch.cuda.synchronize()
    o = obig.cpu()
    assert bool((o[:PAD] == SENT).all()) and bool((o[-PAD:] == SENT).all()), "a write outside out"
    assert torch.equal(big[PAD: PAD + bank_cpu.numel()].cpu(), bank_cpu.reshape(-1)) and bool((big[:PAD] == SENT).all()) \
        and bool((big[-PAD:] == SENT).all()), "the bank or its guards were written"
    return o[PAD: PAD + B * O_ * O_ * 3].view(B, O_, O_, 3), int(err.item())


def _samples(B, S, O_):
    """rows and origins of a batch of B: sample 0 is the LAST bank row with the bottom-right window (it reads the bank's final byte),
    sample 1 the origin (0, 0); the others walk every column origin 0 ... S-O (with S-O >= 15, cx*3 takes every residue mod 16; the
    row pitch S*3 is 8 or 12 mod 16 at the smaller S, so the source addresses do there too) and a stride of row origins; rows descend and repeat."""
    sl = S - O_
    rows = [N_BANK - 1] + [(2 * B - i) % N_BANK for i in range(1, B)]
    crop = [(sl, sl)] + [(0, 0) if i == 1 else ((i * 7 + 3) % (sl + 1), (i - 2) % (sl + 1)) for i in range(1, B)]
    return rows, crop


SHAPES = [(40, 32), (36, 28), (32, 32), (8, 4), (48, 32)]


@pytest.mark.parametrize("S,O_", SHAPES)
def test_bank_batch_is_exact(S, O_):
    bank = _bank(S)
    for B in (1, 3, 70):
        rows, crop = _samples(B, S, O_)
        if B == 70 and S - O_ >= 1:
            assert {c[1] for c in crop} == set(range(S - O_ + 1)) and (0, 0) in crop and (S - O_, S - O_) in crop
        flips = {"none": [0] * B, "all": [1] * B, "mixed": [int(i * 5 % 3 == 0) for i in range(B)], "null": None}
        for tag, flip in flips.items():
            got, err = _run(bank, rows, crop, flip, O_)
            assert err == 0 and torch.equal(got, bank_batch_ref(bank, rows, crop, flip, O_)), (B, tag)
        got, err = _run(bank, rows, None, flips["mixed"], O_)                           # crop_yx NULL: every origin (0, 0)
        assert err == 0 and torch.equal(got, bank_batch_ref(bank, rows, None, flips["mixed"], O_)), (B, "crop null")
        got, err = _run(bank, rows, None, None, O_)
        assert err == 0 and torch.equal(got, bank_batch_ref(bank, rows, None, None, O_)), (B, "both null")
    if S == 48:
        assert {(c[1] * 3) % 16 for c in _samples(70, S, O_)[1]} == set(range(16))      # cx * 3 takes every residue mod 16


def test_bank_batch_at_the_training_shape():
    g = torch.Generator().manual_seed(9)
    bank = torch.randint(0, 256, (3, 256, 256, 3), generator=g, dtype=torch.uint8)
    rows, crop, flip = [2, 0, 2], [(32, 32), (0, 0), (17, 5)], [1, 0, 0]
    got, err = _run(bank, rows, crop, flip, 224)
    assert err == 0 and torch.equal(got, bank_batch_ref(bank, rows, crop, flip, 224))
    got, err = _run(bank, rows, None, None, 256)                                        # the validation transform: a pure gather
    assert err == 0 and torch.equal(got, bank[rows])


def test_bad_entries_keep_the_sentinel_and_are_counted():
    S, O_ = 40, 32
    bank = _bank(S)
    rows, crop, flip = [1, N_BANK, 0, 4, 2], [(0, 0), (1, 1), (8, 8), (3, 9), (2, 2)], [0, 1, 1, 0, 1]     # sample 1: row, sample 3: origin
    got, err = _run(bank, rows, crop, flip, O_)
    assert err == 2
    good = [0, 2, 4]
    want = bank_batch_ref(bank, [rows[i] for i in good], [crop[i] for i in good], [flip[i] for i in good], O_)
    assert torch.equal(got[good], want)
    assert bool((got[[1, 3]] == SENT).all())
    for rows2, crop2 in (([1, -1, 0, 4, 2], [(0, 0), (1, 1), (8, 8), (-1, 0), (2, 2)]), ([1, 2**31 - 1, 0, 4, 2], [(0, 0), (1, 1), (8, 8), (9, 0), (2, 2)])):
        got, err = _run(bank, rows2, crop2, flip, O_)
        assert err == 2 and torch.equal(got[good], want) and bool((got[[1, 3]] == SENT).all())
    # rows the bank holds but the caller's n_rows excludes are bad rows too
    got, err = _run(bank, [0, 3], None, None, O_, n_rows=3)
    assert err == 1 and bool((got[1] == SENT).all()) and torch.equal(got[:1], bank_batch_ref(bank, [0], None, None, O_))


def test_cpu_index_out_of_range_raises_before_any_launch_and_a_device_one_is_counted():
    IB = _IB()
    bank = IB.ImageBank(4, size=8)
    bank.append_resized(_bank(8)[:3])
    names = []
    L = sub("_lib")
    old = L._HOOK[0]
    L._HOOK[0] = lambda name, args: names.append(name)
    try:
        for bad in ([0, 3], [-1, 0], [0, 4]):
            with pytest.raises(IndexError):
                bank.batch(torch.tensor(bad))
        assert names == []
        out = bank.batch(torch.tensor([2, 0, 2]))
        assert names == ["vqa_bank_batch"]
    finally:
        L._HOOK[0] = old
    assert torch.equal(out.data.cpu(), _bank(8)[[2, 0, 2]]) and int(bank.bad_rows) == 0
    assert (list(out.mean), list(out.std)) == (bank.mean, bank.std)
    bank.batch(torch.tensor([0, 3, 1, 7], device=DEV))                                  # a device index is not read back ...
    bank.batch(torch.tensor([5], device=DEV))
    assert int(bank.bad_rows) == 3                                                      # ... the kernel's count accumulates


def test_offsets_into_the_bank_are_64_bit():
    n, S, O_ = 21860, 256, 224
    need = n * S * S * 3
    free = torch.cuda.mem_get_info()[0]
    if free < 8 * 2**30:
        pytest.skip(f"the 64-bit offset test needs a {need / 2**30:.1f} GiB bank; {free / 2**30:.1f} GiB of device memory are free (< 8 GiB)")
    g = torch.Generator().manual_seed(21)
    two = torch.randint(0, 256, (2, S, S, 3), generator=g, dtype=torch.uint8)
    big = torch.empty((n, S, S, 3), dtype=torch.uint8, device=DEV)                       # uninitialised: only two rows are written
    big[3], big[21850] = two[0].to(DEV), two[1].to(DEV)
    assert 21850 * S * S * 3 >= 2**32
    L = sub("_lib")
    rows, crop, flip = [3, 21850, 21850], [(5, 7), (32, 32), (0, 13)], [0, 1, 0]
    out = torch.full((3, O_, O_, 3), SENT, dtype=torch.uint8, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    rows_d, crop_d = torch.tensor(rows, dtype=torch.int32, device=DEV), torch.tensor(crop, dtype=torch.int32, device=DEV)
    flip_d = torch.tensor(flip, dtype=torch.uint8, device=DEV)
    L.call("vqa_bank_batch", big.data_ptr(), n, S, rows_d.data_ptr(), crop_d.data_ptr(), flip_d.data_ptr(), out.data_ptr(), 3, O_,
           err.data_ptr())
    got = out.cpu()
    del big
    torch.cuda.empty_cache()
    assert int(err.item()) == 0
    assert torch.equal(got, bank_batch_ref(two, [0, 1, 1], crop, flip, O_))


# ---------------------------------------------------------------------------------------------------------------- fill
RAGGED = [(480, 640, 1, 5), (100, 150, 2, 5), (37, 1000, 6, 8), (1, 1, 8, 8), (97, 95, 9, 8)]      # sizes of input_oracle.RESIZE_CASES


def _ragged():
    if "ragged" not in _CACHE:
        _CACHE["ragged"] = [torch.from_numpy(IO.pattern_image(h, w, seed, bits)) for h, w, seed, bits in RAGGED]
    return _CACHE["ragged"]


def test_append_equals_the_resizer_and_overflow_leaves_the_bank_alone():
    IB, P = _IB(), _P()
    S = 40
    imgs = _ragged()
    _, want = P.DeviceImageResizer(size=S)(imgs, return_u8=True)
    bank = IB.ImageBank(6, size=S)
    assert bank.append(imgs) == 0 and bank.rows == 5 and bank.nbytes == 6 * S * S * 3
    assert torch.equal(bank.tensor(), want)
    assert np.array_equal(bank.tensor()[0].cpu().numpy(), IO.pil_resize_bilinear(imgs[0].numpy(), S, S))      # the oracle's Resize
    with pytest.raises(ValueError):
        bank.append([imgs[1].to(DEV), imgs[4].to(DEV)])                                 # 5 + 2 > 6
    with pytest.raises(ValueError):
        bank.append_resized(want[:2])
    assert bank.rows == 5 and torch.equal(bank.tensor(), want)
    assert bank.append([imgs[4].to(DEV)]) == 5 and bank.rows == 6                        # device images, and the returned first row
    assert torch.equal(bank.tensor()[5], want[4]) and torch.equal(bank.tensor()[:5], want)
    with pytest.raises(RuntimeError):
        bank.append([imgs[0].float()])


def test_append_works_in_chunks_of_64():
    IB, P = _IB(), _P()
    g = torch.Generator().manual_seed(2)
    imgs = [torch.randint(0, 256, (5 + i % 4, 9 - i % 3, 3), generator=g, dtype=torch.uint8) for i in range(70)]
    bank = IB.ImageBank(70, size=8)
    names = []
    L = sub("_lib")
    old = L._HOOK[0]
    L._HOOK[0] = lambda name, args: names.append((name, args[5]))                        # vqa_image_resize's n
    try:
        assert bank.append(imgs) == 0
    finally:
        L._HOOK[0] = old
    assert names == [("vqa_image_resize", 64), ("vqa_image_resize", 6)]
    _, want = P.DeviceImageResizer(size=8)(imgs[:64], return_u8=True)
    _, tail = P.DeviceImageResizer(size=8)(imgs[64:], return_u8=True)
    assert torch.equal(bank.tensor(), torch.cat([want, tail]))


# ---------------------------------------------------------------------------------------------------------------- whole transform
def test_batch_equals_the_resizer_route_and_the_oracle():
    IB, P = _IB(), _P()
    imgs = _ragged()
    jitter = P.DeviceColorJitter(0.2, 0.2, 0.2, 0.1)
    bank = IB.ImageBank(5, size=40)
    bank.append(imgs)
    crop_yx, flip = [(8, 8), (0, 0), (3, 5), (7, 1), (0, 8)], torch.tensor([1, 0, 1, 1, 0], dtype=torch.bool)
    params = jitter.draw(5, torch.Generator().manual_seed(3))
    want = P.DeviceImageResizer(size=40, crop=32, jitter=jitter)(imgs, crop_yx=crop_yx, flip=flip, jitter_params=params, output="bytes")
    got = bank.batch(torch.arange(5), crop=32, crop_yx=crop_yx, flip=flip, jitter=jitter, jitter_params=params)
    assert got.data.shape == (5, 32, 32, 3) and torch.equal(got.data, want.data)
    # without the jitter: the other existing route, and the oracle (full Resize, then crop, then flip), which decides
    want = P.DeviceImageResizer(size=40, crop=32)(imgs, crop_yx=crop_yx, flip=flip, output="bytes")
    got = bank.batch(torch.arange(5), crop=32, crop_yx=crop_yx, flip=flip)
    assert torch.equal(got.data, want.data)
    for b in range(5):
        x = IO.pil_resize_bilinear(imgs[b].numpy(), 40, 40)[crop_yx[b][0]: crop_yx[b][0] + 32, crop_yx[b][1]: crop_yx[b][1] + 32]
        x = x[:, ::-1] if bool(flip[b]) else x
        assert np.array_equal(got.data[b].cpu().numpy(), x), b
    # and the jitter on top of the oracle's bytes, by the oracle's ColorJitter
    order, factors = params
    got = bank.batch(torch.tensor([2]), crop=32, crop_yx=[crop_yx[2]], flip=flip[2:3], jitter=jitter, jitter_params=(order[2:3], factors[2:3]))
    x = IO.pil_resize_bilinear(imgs[2].numpy(), 40, 40)[3:35, 5:37][:, ::-1]
    f = [float(v) for v in factors[2]]
    assert np.array_equal(got.data[0].cpu().numpy(), IO.color_jitter(x, [int(v) for v in order[2]], *f))


def test_batch_with_one_generator_state_equals_gpu_collate_fn():
    IB, P = _IB(), _P()
    imgs = _ragged()
    jitter = P.DeviceColorJitter(0.2, 0.2, 0.2, 0.1)
    bank = IB.ImageBank(5, size=40)
    bank.append(imgs)
    items = [(im, torch.zeros(4, dtype=torch.long), torch.ones(4, dtype=torch.long), i) for i, im in enumerate(imgs)]
    for seed in (5, 6):
        g1, g2 = torch.Generator().manual_seed(seed), torch.Generator().manual_seed(seed)
        want = P.gpu_collate_fn(items, flip_p=0.5, generator=g1, resizer=P.DeviceImageResizer(size=40, crop=32, jitter=jitter), output="bytes")
        got = bank.batch(torch.arange(5), crop=32, flip_p=0.5, jitter=jitter, generator=g2)
        assert torch.equal(got.data, want["images"].data) and torch.equal(g1.get_state(), g2.get_state()), seed
    # the validation transform: a bank of the final size, no crop -- a pure gather
    val = IB.ImageBank(5, size=32)
    val.append(imgs)
    want = P.DeviceImageResizer(size=32)(imgs, output="bytes")
    assert torch.equal(val.batch(torch.tensor([4, 1, 1])).data, want.data[[4, 1, 1]])


def test_a_draw_is_two_launches_and_jitter_parameters_are_checked():
    IB, P = _IB(), _P()
    jitter = P.DeviceColorJitter(0.2, 0.2, 0.2, 0.1)
    bank = IB.ImageBank(5, size=8)
    bank.append_resized(_bank(8))
    names = []
    L = sub("_lib")
    old = L._HOOK[0]
    L._HOOK[0] = lambda name, args: names.append(name)
    try:
        bank.batch(torch.arange(5), crop=4, flip_p=0.5, jitter=jitter, generator=torch.Generator().manual_seed(1))
        assert names == ["vqa_bank_batch", "vqa_image_color_jitter"]
        order, factors = jitter.draw(5, torch.Generator().manual_seed(2))
        factors[3, 3] = 0.6
        with pytest.raises(ValueError, match="hue_factor"):
            bank.batch(torch.arange(5), jitter=jitter, jitter_params=(order, factors))
        with pytest.raises(RuntimeError, match="one row per sample"):
            bank.batch(torch.arange(5), jitter=jitter, jitter_params=(order[:4], factors[:4]))
        assert len(names) == 2                                                          # refused before any launch
    finally:
        L._HOOK[0] = old


# ---------------------------------------------------------------------------------------------------------------- loader
def _table(N=23, U=7, L_=6, seed=4):
    g = torch.Generator().manual_seed(seed)
    image_row = torch.randint(0, U, (N,), generator=g)
    image_row[:U] = torch.arange(U)                                                      # every image is used
    ids = torch.randint(0, 100, (N, L_), generator=g)
    ids[:, 0] = torch.arange(N)                                                          # column 0 names the sample
    mask = (torch.rand(N, L_, generator=g) < 0.7).long()
    answers = torch.randint(0, 10, (N,), generator=g)
    return image_row, ids, mask, answers


@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "group_by_image"])
def test_loader_yields_every_sample_once_and_direct_gathers(grouped):
    IB = _IB()
    image_row, ids, mask, answers = _table()
    src = _bank(8, seed=1)
    src = torch.cat([src, src.flip(0)[:2].roll(1, 1)])                                   # 7 distinct 8 x 8 images
    bank = IB.ImageBank(7, size=8)
    bank.append_resized(src)
    loader = IB.BankLoader(bank, image_row, ids, mask, answers, batch_size=5, seed=3, group_by_image=grouped)
    assert len(loader) == 5
    seen = []
    for batch in loader:
        assert set(batch) == {"images", "token_ids", "attention_mask", "answers"} | ({"image_index"} if grouped else set())
        idx = batch["token_ids"][:, 0].cpu()
        seen += idx.tolist()
        assert batch["token_ids"].dtype == batch["attention_mask"].dtype == batch["answers"].dtype == torch.int64
        assert torch.equal(batch["token_ids"].cpu(), ids[idx]) and torch.equal(batch["attention_mask"].cpu(), mask[idx])
        assert torch.equal(batch["answers"].cpu(), answers[idx])
        data = batch["images"].data
        if grouped:
            assert data.shape[0] == len(set(image_row[idx].tolist()))
            assert batch["image_index"].dtype == torch.int64
            data = data[batch["image_index"].to(DEV)]
        assert torch.equal(data.cpu(), src[image_row[idx]])
    assert sorted(seen) == list(range(23))
    loader.set_epoch(1)
    again = [b["token_ids"][:, 0].cpu() for b in loader]
    assert sorted(torch.cat(again).tolist()) == list(range(23)) and torch.cat(again).tolist() != seen
    assert int(bank.bad_rows) == 0


def test_loader_draws_once_per_image_soft_targets_and_resume():
    IB, P = _IB(), _P()
    ST = pkg().load_dropin_soft_targets().SoftTargets
    image_row, ids, mask, _ = _table()
    g = torch.Generator().manual_seed(8)
    soft = ST(torch.randint(-1, 10, (23, 3), generator=g, dtype=torch.int32), torch.rand(23, 3, generator=g),
              torch.randint(0, 4, (23, 3), generator=g, dtype=torch.int32))
    src = _bank(16, seed=2)
    src = torch.cat([src, src.flip(0)[:2].roll(1, 2)])
    bank = IB.ImageBank(7, size=16)
    bank.append_resized(src)
    jitter = P.DeviceColorJitter(0.2, 0.2, 0.2, 0.1)
    kw = dict(batch_size=5, seed=3, crop=12, flip_p=0.5, jitter=jitter, group_by_image=True)
    loader = IB.BankLoader(bank, image_row, ids, mask, soft, **kw)
    batches, state = [], None
    for k, b in enumerate(loader):
        idx = b["token_ids"][:, 0].cpu()
        assert isinstance(b["answers"], ST)
        assert torch.equal(b["answers"].ids.cpu(), soft.ids[idx]) and torch.equal(b["answers"].weights.cpu(), soft.weights[idx])
        assert torch.equal(b["answers"].counts.cpu(), soft.counts[idx])
        assert b["images"].data.shape[1:] == (12, 12, 3) and b["images"].data.shape[0] == int(b["image_index"].max()) + 1
        batches.append((idx, b["images"].data.cpu(), b["image_index"].clone()))
        if k == 1:
            state = loader.state_dict()
    # the draws come from the sampler's generator, one per image: the same loader state gives the same bytes
    twin = IB.BankLoader(bank, image_row, ids, mask, soft, **kw)
    twin.load_state_dict(state)
    rest = [(b["token_ids"][:, 0].cpu(), b["images"].data.cpu(), b["image_index"]) for b in twin]
    assert len(rest) == 3
    for x, y in zip(rest, batches[2:]):
        assert all(torch.equal(p, q) for p, q in zip(x, y))


# ---------------------------------------------------------------------------------------------------------------- into the trainer
SMALL = dict(vocab_size=100, num_answers=10, embed_dim=32)
CFG = O.full_config(dropout=0.1, answer_dropout=0.1, **SMALL)


def _model():
    if "sd" not in _CACHE:
        _CACHE["sd"] = O.init_state_dict(CFG, 41, jitter=True)
    m = pkg().load_dropin().VQAModel(**CFG, compute_dtype="bf16")
    m.load_state_dict(_CACHE["sd"])
    return m.to(DEV).train()


@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "image_index"])
def test_trainer_step_on_a_loader_batch_equals_the_step_on_the_same_bytes(grouped):
    IB = _IB()
    BI = pkg().load_dropin_byte_images().ByteImages
    T = pkg().trainer.HipTrainer
    N, U = 12, 4
    _, ids, mask, answers = O.synthetic_batch(N, seed=6, image_size=64, seq_len=10, vocab=100, num_answers=10)
    image_row = torch.tensor([0, 1, 1, 0, 2, 0, 2, 3, 3, 1, 2, 0])
    bank = IB.ImageBank(U, size=80)
    bank.append_resized(R.images(U, 80, 80, seed=3))
    loader = IB.BankLoader(bank, image_row, ids, mask, answers, batch_size=6, seed=1, crop=64, flip_p=0.5, group_by_image=grouped)
    a, b = _model(), _model()
    ta, tb = T(a, lr=1e-3), T(b, lr=1e-3)
    steps = 0
    for batch in loader:
        images = batch["images"]
        index = batch.get("image_index")
        assert images.data.shape == ((len(set(index.tolist())) if grouped else 6), 64, 64, 3)
        hand = BI(images.data.clone(), images.mean, images.std)
        la, lga = ta.step(images, batch["token_ids"], batch["attention_mask"], batch["answers"], image_index=index)
        lb, lgb = tb.step(hand, batch["token_ids"].clone(), batch["attention_mask"].clone(), batch["answers"].clone(),
                          image_index=None if index is None else index.clone())
        torch.cuda.synchronize()
        assert bool(torch.isfinite(la).all())
        assert torch.equal(la, lb) and torch.equal(lga, lgb) and torch.equal(a._flat, b._flat), steps
        steps += 1
    assert steps == 2
