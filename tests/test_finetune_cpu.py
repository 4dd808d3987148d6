"""Fine-tuning with frozen parts, host side: the optimizer's trainable-range table, the backward plan, the per-part mode resolution
and the reducer's group selection (gloo CPU rehearsal).  No GPU."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from _pkg import pkg, sub
from oracle import vqa_oracle as O

CFG = O.full_config(embed_dim=32, vocab_size=100, num_answers=10)


def _entries():
    LY = sub("layout")
    return [e for e in LY.build_entries(CFG) if e.is_param]


def _mask(pents, pred):
    return tuple(bool(pred(e.name)) for e in pents)


def _covered(ranges):
    return sum(hi - lo for lo, hi, _ in ranges)


def test_range_table_patterns():
    FT, LY = sub("finetune"), sub("layout")
    pe = _entries()
    slot = lambda e: (e.numel + LY.ALIGN - 1) // LY.ALIGN * LY.ALIGN
    # everything: one range over every parameter slot
    r = FT.trainable_ranges(pe, (True,) * len(pe))
    assert len(r) == 1 and r[0][0] == pe[0].offset and r[0][1] == FT.slot_end(pe[-1]) and r[0][2] == 0
    # nothing
    assert FT.trainable_ranges(pe, (False,) * len(pe)) == []
    assert FT.range_table_rows([]) == []
    # CNN frozen: the token-side parameters only, merged where adjacent
    m = _mask(pe, lambda n: not n.startswith("image_encoder."))
    r = FT.trainable_ranges(pe, m)
    assert _covered(r) == sum(slot(e) for e, t in zip(pe, m) if t)
    cnn = [e for e in pe if e.name.startswith("image_encoder.")]
    for lo, hi, _ in r:
        assert not any(lo < FT.slot_end(e) and e.offset < hi for e in cnn)
    # a single middle parameter
    j = len(pe) // 2
    m = tuple(i == j for i in range(len(pe)))
    assert FT.trainable_ranges(pe, m) == [(pe[j].offset, FT.slot_end(pe[j]), j)]
    # the embedding only
    k = [e.name for e in pe].index("text_encoder.token_embedding.weight")
    m = tuple(i == k for i in range(len(pe)))
    r = FT.trainable_ranges(pe, m)
    assert r == [(pe[k].offset, FT.slot_end(pe[k]), k)]
    rows = FT.range_table_rows(r)
    assert rows == [[pe[k].offset, FT.slot_end(pe[k]), 0, k]]
    # every bound the kernels read is a multiple of 4 (float4 loads)
    m = tuple(i % 3 == 0 for i in range(len(pe)))
    for lo, hi, pos, _ in FT.range_table_rows(FT.trainable_ranges(pe, m)):
        assert lo % 4 == 0 and hi % 4 == 0 and pos % 4 == 0


def test_lag_classes_split_merged_ranges():
    """Parameters frozen during different steps carry different Adam step counts: never one range."""
    FT = sub("finetune")
    pe = _entries()
    n = len(pe)
    cls = [0] * n
    cls = FT.refine_classes(cls, tuple(i != 1 for i in range(n)))     # parameter 1 frozen for a while
    cls = FT.refine_classes(cls, (True,) * n)                          # then everything trains again
    r = FT.trainable_ranges(pe, (True,) * n, cls)
    assert [x[2] for x in r] == [0, 1, 2]
    assert _covered(r) == FT.slot_end(pe[-1]) - pe[0].offset


def _plan(pred, modes=(True,) * 4, images_grad=False):
    FT = sub("finetune")
    pe = _entries()
    return FT.Plan(pe, _mask(pe, pred), modes, images_grad)


def test_backward_plan_patterns():
    allp = _plan(lambda n: True)
    assert allp.cnn_tape and allp.cnn_low == 0 and allp.text and allp.fusion_bwd and allp.need_dfused
    assert allp.cnn_levels()[-1] == "image_encoder.stem"

    none = _plan(lambda n: False)
    assert not none.cnn_tape and none.cnn_low is None and not none.text and not none.fusion_bwd and not none.need_dfused

    cnn_frozen = _plan(lambda n: not n.startswith("image_encoder."))
    assert not cnn_frozen.cnn_tape and cnn_frozen.cnn_low is None and cnn_frozen.cnn_levels() == []
    assert cnn_frozen.text and cnn_frozen.fusion_bwd and not cnn_frozen.need_dfeat and cnn_frozen.need_denc

    s12 = _plan(lambda n: not (n.startswith("image_encoder.stage1.") or n.startswith("image_encoder.stage2.")
                               or n.startswith("image_encoder.stem.")))
    assert s12.cnn_tape and s12.cnn_low == 3
    assert s12.cnn_levels() == ["image_encoder.stage4", "image_encoder.stage3"]

    head_fusion = _plan(lambda n: n.startswith("answer_head.") or n.startswith("fusion."))
    assert head_fusion.fusion_bwd and not head_fusion.text and head_fusion.cnn_low is None and not head_fusion.need_dfeat

    head_only = _plan(lambda n: n.startswith("answer_head."))
    assert not head_only.fusion_bwd and not head_only.need_dfused

    emb = _plan(lambda n: n == "text_encoder.token_embedding.weight")
    assert emb.text and emb.fusion_bwd and emb.cnn_low is None

    saliency = _plan(lambda n: False, images_grad=True)
    assert saliency.cnn_tape and saliency.cnn_low == 0 and saliency.need_dfused and not saliency.text

    # a middle parameter frozen: its slot is skipped, its neighbours are not
    pe = _entries()
    j = len(pe) // 2
    FT = sub("finetune")
    mid = FT.Plan(pe, tuple(i != j for i in range(len(pe))), (True,) * 4, False)
    assert mid.frozen(pe[j].offset, pe[j].numel)
    assert not mid.frozen(pe[j - 1].offset, pe[j - 1].numel) and not mid.frozen(pe[j + 1].offset, pe[j + 1].numel)
    assert not mid.frozen(pe[j].offset, pe[j].numel + FT.slot_end(pe[j + 1]) - pe[j].offset)


def test_resolve_keeps_the_plain_route_and_caches():
    FT = sub("finetune")
    pe = _entries()

    class P:
        def __init__(self, rg):
            self.requires_grad = rg

    params = [P(True) for _ in pe]
    assert FT.resolve(pe, params, (True,) * 4, False) is None
    assert FT.resolve(pe, params, (False,) * 4, True) is None
    cache = {}
    a = FT.resolve(pe, params, (False, True, True, True), False, cache)
    assert a is not None and a.modes == (False, True, True, True) and all(a.trainable)
    assert FT.resolve(pe, params, (False, True, True, True), False, cache) is a
    params[0].requires_grad = False
    b = FT.resolve(pe, params, (True,) * 4, False, cache)
    assert b is not a and not b.trainable[0]


def test_part_modes_and_mixed_mode_inside_a_part():
    m = pkg().load_dropin().VQAModel(**CFG, compute_dtype="fp32")
    FT = sub("finetune")
    m.train()
    assert FT.part_modes(m) == (True, True, True, True) and m._part_modes() == (True, True, True, True)
    m.image_encoder.eval()
    assert FT.part_modes(m) == (False, True, True, True) and m._part_modes() == (False, True, True, True)
    m.eval()
    m.fusion.train()
    assert m._part_modes() == (False, False, True, False)
    m.train()
    m.image_encoder.stage3.eval()
    with pytest.raises(NotImplementedError, match="image_encoder.stage3"):
        m._part_modes()
    m.train()
    m.answer_head.classifier.eval()
    with pytest.raises(NotImplementedError, match="answer_head.classifier"):
        FT.part_modes(m)
    # the plan follows requires_grad; a model that trains everything in one mode keeps the plain route
    m.train()
    params = m._param_list()
    assert m._finetune_plan(params, False, True) is None
    m.image_encoder.requires_grad_(False)
    pl = m._finetune_plan(params, False, True)
    assert pl is not None and pl.cnn_low is None and not pl.cnn_tape
    assert m._finetune_plan(params, False, True) is pl           # unchanged trainable set and modes: the cached plan


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    LY, TR, FT = sub("layout"), sub("trainer"), sub("finetune")
    ent = LY.build_entries(CFG)
    pe = [e for e in ent if e.is_param]
    n = LY.flat_size(ent)
    G = torch.randn(n, generator=torch.Generator().manual_seed(100 + rank))
    mine = G.clone()
    red = TR.GradBucketReducer(G, LY.bucket_ranges(ent))
    # the CNN frozen on every rank: only the token-side group travels
    red.set_trainable(FT.trainable_ranges(pe, tuple(not e.name.startswith("image_encoder.") for e in pe)))
    bad = torch.tensor([rank + 1], dtype=torch.int32)
    red.reduce_aux(bad)
    for name, _, _ in red.buckets:
        red.on_segment(name)
    issued = list(red.issued)
    red.finish()
    others = [torch.randn(n, generator=torch.Generator().manual_seed(100 + r)) for r in range(world)]
    expect = sum(others)
    lo, hi = red.groups[0][1], red.groups[0][2]
    ok = (torch.allclose(G[lo:hi], expect[lo:hi], atol=1e-6) and torch.equal(G[hi:], mine[hi:]) and int(bad) == sum(range(1, world + 1)))
    # everything trains again: every group travels
    red.set_trainable(None)
    for name, _, _ in red.buckets:
        red.on_segment(name)
    issued_all = list(red.issued)
    red.finish()
    q.put((rank, bool(ok), issued, issued_all))
    dist.destroy_process_group()


def test_reducer_sends_only_trainable_groups_gloo():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in ps:
        p.join(timeout=60)
        assert p.exitcode == 0
    for _, ok, issued, issued_all in res:
        assert ok
        assert issued == ["answer_head+fusion+text_encoder"]
        assert len(issued_all) == 4
