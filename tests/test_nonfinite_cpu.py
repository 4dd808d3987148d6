"""CPU: the host side of HipTrainer's non-finite guard -- the option's validation, the "hip_trainer" block's new fields through
trainer_state.export / load in every direction, and the guard flag in the captured step's key."""
import inspect

import pytest
import torch

from _pkg import sub
from oracle import vqa_oracle as O

CFG = O.full_config(vocab_size=50, num_answers=7, embed_dim=32)


def _ts():
    return sub("trainer_state")


def _entries():
    return [e for e in sub("layout").build_entries(CFG) if e.is_param]


def _flat(entries, seed):
    LY = sub("layout")
    flat = torch.zeros(LY.flat_size(entries))
    g = torch.Generator().manual_seed(seed)
    for e in entries:
        LY.view_of(flat, e).copy_(torch.randn(e.shape, generator=g))
    return flat


def _export(entries, **kw):
    n = len(entries)
    args = dict(calls=9, skipped_ever=3, bad_targets=[2, 1], empty=0, lag=[0] * n, lag_class=[0] * n, ever_frozen=False, lr=2e-4,
                betas=(0.9, 0.98), eps=1e-7, weight_decay=0.05, max_grad_norm=2.0, groups=None, ema=None, ema_decay=None, ema_warmup=False,
                seed_base=0x5EED, step_id=9)
    args.update(kw)
    return _ts().export(entries, [e.name for e in entries], _flat(entries, 1), _flat(entries, 2).square(), **args)


def _load(entries, sd):
    return _ts().load(entries, [e.name for e in entries], sd, _flat(entries, 11), _flat(entries, 12), None, None)


def test_the_option_takes_none_skip_and_raise():
    TS = _ts()
    assert [TS.check_nonfinite(v) for v in (None, "skip", "raise")] == [None, "skip", "raise"]
    for bad in ("Skip", "", "ignore", True, False, 0, 1, ("skip",), b"skip"):
        with pytest.raises(ValueError, match="nonfinite"):
            TS.check_nonfinite(bad)


def test_the_constructor_validates_the_option_before_it_touches_the_model():
    T = sub("trainer").HipTrainer
    assert inspect.signature(T.__init__).parameters["nonfinite"].default is None
    with pytest.raises(ValueError, match="nonfinite"):
        T(object(), nonfinite="warn")                      # (a model would be needed only after the check)


def test_without_the_guard_the_block_has_the_keys_it_had():
    entries = _entries()
    sd = _export(entries)
    assert "nonfinite" not in sd["hip_trainer"]
    assert _load(entries, sd)["nonfinite"] is None


@pytest.mark.parametrize("mode", ["skip", "raise"])
def test_the_block_round_trips_the_new_fields(mode):
    entries = _entries()
    sd = _export(entries, nonfinite=mode, nonfinite_skipped=(1, 2, 2))
    block = sd["hip_trainer"]
    assert block["nonfinite"] == {"mode": mode, "since": 1, "ever": 2, "unchecked": 2}
    assert block["skipped_ever"] == 3 and block["bad_targets"] == [2, 1]                 # every launch that was no step, untouched
    assert [int(s["step"]) for s in sd["state"].values()] == [6] * len(entries)          # steps_of: calls - skipped_ever
    r = _load(entries, sd)
    assert r["nonfinite"] == block["nonfinite"] and r["skipped_ever"] == 3 and r["calls"] == 9
    import io
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    assert torch.load(buf, weights_only=True)["hip_trainer"]["nonfinite"] == block["nonfinite"]


def test_load_refuses_counters_that_do_not_fit():
    entries = _entries()
    for skipped in ((1, 4, 0), (3, 2, 0), (0, 2, 3)):      # more non-finite skips than skipped launches; since / unchecked above ever
        sd = _export(entries, nonfinite="skip", nonfinite_skipped=skipped)
        with pytest.raises(ValueError, match="nonfinite"):
            _load(entries, sd)
    sd = _export(entries, nonfinite="skip")
    sd["hip_trainer"]["nonfinite"]["mode"] = "warn"
    with pytest.raises(ValueError, match="nonfinite"):
        _load(entries, sd)
    with pytest.raises(ValueError, match="nonfinite"):
        _export(entries, nonfinite="warn")


def test_the_guard_flag_is_part_of_the_step_key():
    SG = sub("stepgraph")
    assert SG.table_id(None) is None and SG.table_id(7) == 7 and SG.table_id(7, None, False) == 7
    ids = [SG.table_id(None), SG.table_id(7), SG.table_id(7, [0, 1]), SG.table_id(None, guard=True), SG.table_id(7, guard=True),
           SG.table_id(7, [0, 1], guard=True)]
    assert len(set(ids)) == len(ids)
    kw = dict(features=True, images=torch.zeros(4, 2, 2, 512), token_ids=torch.zeros(4, 10, dtype=torch.long), attention_mask=None,
              image_index=None, targets=torch.zeros(4, dtype=torch.long), plan=None, loss_kind="ce", loss_opts=(0.0, None, None), ema=False,
              metrics=None, flat_ptr=0x1000, wsrc_ptr=0x2000)
    assert SG.step_key(**kw, table_id=SG.table_id(None)) != SG.step_key(**kw, table_id=SG.table_id(None, guard=True))
