"""CPU: the host logic behind cached image features -- what keeps an ImageFeatures valid and what makes it stale (the integers of
VQAModel._feat_stamp that do not need an engine), the index check of ImageFeatures.select, and the plan flag the trainer reads."""
import pytest
import torch

from _pkg import pkg, sub
from oracle import vqa_oracle as O

CFG = O.full_config(vocab_size=100, num_answers=10, embed_dim=32)


def _model():
    m = pkg().load_dropin().VQAModel(**CFG, compute_dtype="fp32", seed=5)
    m._feat_live = True          # as after encode_features / features_from_tensor: the optimizer step hooks look at this model
    return m


def _host_stamp(m):
    return (m._feat_epoch, m._feat_version() - m._feat_excused)


def _give_grads(params):
    for p in params:
        p.grad = torch.full_like(p, 1e-3)


def test_optimizer_steps_on_the_other_parts_leave_the_stamp_alone():
    m = _model()
    m.image_encoder.requires_grad_(False)
    s0, flat0 = _host_stamp(m), m._flat.clone()
    rest = [p for p in m.parameters() if p.requires_grad]
    opt = torch.optim.AdamW(rest, lr=1e-2)
    for _ in range(2):
        _give_grads(rest)
        opt.step()
    assert not torch.equal(flat0, m._flat) and _host_stamp(m) == s0
    # an optimizer that holds the frozen image-encoder parameters too, none of them with a gradient
    opt = torch.optim.SGD(list(m.parameters()), lr=1e-2)
    opt.step()
    assert _host_stamp(m) == s0


def test_whatever_changes_the_image_encoder_moves_the_stamp():
    m = _model()
    cnn = list(m.image_encoder.parameters())
    assert len(cnn) == len(m._cnn_params()) and all(a is b for a, b in zip(cnn, m._cnn_params()))
    s = _host_stamp(m)
    opt = torch.optim.SGD(list(m.parameters()), lr=1e-2)        # a step that writes an image-encoder parameter
    _give_grads(cnn[:1])
    opt.step()
    assert _host_stamp(m) != s
    s = _host_stamp(m)
    with torch.no_grad():                                       # an in-place torch write
        cnn[3].add_(0)
    assert _host_stamp(m) != s
    s = _host_stamp(m)
    m.load_state_dict(m.state_dict())
    assert _host_stamp(m)[0] > s[0]
    s = _host_stamp(m)
    m.to(torch.float32)                                         # (_apply re-flattens the parameters)
    assert _host_stamp(m)[0] > s[0]
    s = _host_stamp(m)
    m.invalidate_features()
    assert _host_stamp(m)[0] > s[0]


def test_ema_exchange_keeps_the_stamp_only_when_told_the_cnn_is_the_same():
    m = _model()
    ema = m._flat.detach().clone()
    s = _host_stamp(m)
    with sub("ema").swapped(m, ema, keeps_cnn=True):
        assert _host_stamp(m) == s
    assert _host_stamp(m) == s
    with sub("ema").swapped(m, ema):
        assert _host_stamp(m) != s
    assert _host_stamp(m) != s


def test_select_index_check():
    M = pkg().load_dropin()
    ok = M._checked_index(torch.tensor([2, 0, 2], dtype=torch.int32), 3, "index")
    assert ok.tolist() == [2, 0, 2]
    assert M._checked_index([1, 0], 2, "index").tolist() == [1, 0]
    assert M._checked_index(torch.zeros(0, dtype=torch.long), 0, "index").numel() == 0
    for bad in (torch.tensor([0, 3]), torch.tensor([-1, 0])):
        with pytest.raises(IndexError):
            M._checked_index(bad, 3, "index")
    for bad in (torch.tensor([0.0]), torch.tensor([True]), torch.tensor([[0]]), torch.tensor(1)):
        with pytest.raises(ValueError):
            M._checked_index(bad, 3, "index")


def test_features_cat_and_wrapping_checks():
    M = pkg().load_dropin()
    m = _model()
    a = M.ImageFeatures(torch.zeros(2, 2, 2, 512), (0, 0, 0), m._handle)
    b = M.ImageFeatures(torch.ones(1, 2, 2, 512), (0, 0, 0), m._handle)
    c = M.ImageFeatures.cat([a, b])
    assert c.num_images == 3 and torch.equal(c.tensor()[2], torch.ones(2, 2, 512))
    with pytest.raises(RuntimeError):
        M.ImageFeatures.cat([a, M.ImageFeatures(torch.ones(1, 2, 2, 512), (1, 0, 0), m._handle)])
    with pytest.raises(ValueError):
        M.ImageFeatures.cat([])
    for bad in (torch.zeros(2, 2, 512), torch.zeros(1, 2, 2, 64), torch.zeros(1, 2, 2, 512, dtype=torch.bfloat16)):
        with pytest.raises(ValueError):
            m.features_from_tensor(bad)


def test_plan_says_whether_the_image_encoder_trains():
    FT = sub("finetune")
    m = _model()
    ents = m._param_entries
    frozen_cnn = tuple(not e.name.startswith("image_encoder.") for e in ents)
    assert not FT.Plan(ents, frozen_cnn, (False, True, True, True), False).cnn_trains
    assert not FT.Plan(ents, frozen_cnn, (False, True, True, True), True).cnn_trains       # an image gradient trains nothing
    one = tuple(t or e.name == "image_encoder.stage4.blocks.1.conv2.weight" for t, e in zip(frozen_cnn, ents))
    assert FT.Plan(ents, one, (False, True, True, True), False).cnn_trains
