"""Parameter groups of HipTrainer, host side: which parameter lands in which group (names, prefixes, Parameter objects, the implicit
last group, every refusal), no_weight_decay_groups, the range table under group boundaries, the ctypes view of vqa_group_hyper and
the key a captured step is filed under.  No GPU."""
import ctypes
import os
import re

import pytest
import torch

from _pkg import REPO, pkg, sub
from oracle import vqa_oracle as O

CFG = O.full_config(vocab_size=100, num_answers=10, embed_dim=32)


def _entries(cfg=CFG):
    return [e for e in sub("layout").build_entries(cfg) if e.is_param]


class _P:
    """stands in for an nn.Parameter: only its identity is read"""


def _resolve(spec, pe=None, params=None):
    pe = _entries() if pe is None else pe
    params = [_P() for _ in pe] if params is None else params
    return sub("finetune").ParamGroups(pe, params, spec)


# ------------------------------------------------------------------------------------------------------------ group resolution
def test_names_prefixes_and_parameter_objects_resolve_and_the_rest_is_implicit():
    pe = _entries()
    names = [e.name for e in pe]
    m = pkg().load_dropin().VQAModel(**CFG, compute_dtype="fp32")
    params = m._param_list()
    assert [e.name for e in m._param_entries] == names
    head_w = dict(m.named_parameters())["answer_head.classifier.0.weight"] if "answer_head.classifier.0.weight" in names else params[-1]
    j_obj = next(j for j, p in enumerate(params) if p is head_w)
    pg = _resolve([{"params": ["image_encoder."], "lr_scale": 0.1},
                   {"params": ["text_encoder.token_embedding.weight", head_w], "weight_decay": 0.0}], pe, params)
    assert len(pg.groups) == 3
    g0, g1, rest = pg.groups
    assert g0["names"] == tuple(n for n in names if n.startswith("image_encoder.")) and g0["lr_scale"] == 0.1 and g0["weight_decay"] is None
    assert set(g1["names"]) == {"text_encoder.token_embedding.weight", names[j_obj]} and g1["lr_scale"] == 1.0 and g1["weight_decay"] == 0.0
    assert rest["lr_scale"] == 1.0 and rest["weight_decay"] is None                # what no group selected
    assert sorted(g0["names"] + g1["names"] + rest["names"]) == sorted(names)
    assert pg.group_of == pg.key() and len(pg.group_of) == len(names)
    for gi, g in enumerate(pg.groups):
        assert all(pg.group_of[names.index(n)] == gi for n in g["names"])
    # every parameter selected: no implicit group; a bare string is one selector
    pg = _resolve([{"params": "image_encoder."}, {"params": [n for n in names if not n.startswith("image_encoder.")]}])
    assert len(pg.groups) == 2
    # the values of the live dicts: None follows the trainer's weight decay
    pg = _resolve([{"params": ["fusion."], "lr_scale": 2.0, "weight_decay": 0.5}])
    assert pg.effective(0.01) == ((2.0, 1.0), (0.5, 0.01))
    pg.groups[1]["lr_scale"] = 0.0
    assert pg.effective(0.2) == ((2.0, 0.0), (0.5, 0.2))


def test_refusals():
    pe = _entries()
    params = [_P() for _ in pe]
    name = pe[3].name
    with pytest.raises(KeyError):
        _resolve([{"params": ["image_encoder.no_such.weight"]}], pe, params)
    with pytest.raises(KeyError):
        _resolve([{"params": ["no_such_part."]}], pe, params)
    with pytest.raises(KeyError):
        _resolve([{"params": ["image_encoder"]}], pe, params)                     # a prefix ends in "."
    with pytest.raises(ValueError, match=re.escape(name)):
        _resolve([{"params": [name]}, {"params": ["image_encoder."]}], pe, params)   # in two groups: named
    with pytest.raises(ValueError, match=re.escape(name)):
        _resolve([{"params": [name, params[3]]}], pe, params)
    with pytest.raises(ValueError):
        _resolve([{"params": [torch.nn.Parameter(torch.zeros(2))]}], pe, params)   # not this model's
    with pytest.raises(ValueError):
        _resolve([{"params": []}], pe, params)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            _resolve([{"params": ["fusion."], "lr_scale": bad}], pe, params)
        with pytest.raises(ValueError):
            _resolve([{"params": ["fusion."], "weight_decay": bad}], pe, params)
    # a bad live value, or a bad trainer weight decay behind a None
    pg = _resolve([{"params": ["fusion."]}], pe, params)
    pg.groups[0]["lr_scale"] = float("nan")
    with pytest.raises(ValueError):
        pg.effective(0.01)
    pg.groups[0]["lr_scale"] = 1.0
    pg.groups[0]["weight_decay"] = -0.1
    with pytest.raises(ValueError):
        pg.effective(0.01)
    pg.groups[0]["weight_decay"] = None
    with pytest.raises(ValueError):
        pg.effective(float("inf"))


def test_sixteen_groups_pass_and_seventeen_are_refused():
    pe = _entries()
    assert len(pe) >= 17
    pg = _resolve([{"params": [pe[j].name]} for j in range(15)])                  # 15 + the implicit one
    assert len(pg.groups) == 16
    _resolve([{"params": [pe[j].name]} for j in range(15)] + [{"params": [e.name for e in pe[15:]]}])      # 16, nothing left over
    with pytest.raises(ValueError, match="17"):
        _resolve([{"params": [pe[j].name]} for j in range(16)])                   # 16 + the implicit one
    with pytest.raises(ValueError, match="17"):
        _resolve([{"params": [pe[j].name]} for j in range(16)] + [{"params": [e.name for e in pe[16:]]}])


def test_a_table_of_more_than_512_rows_is_refused_with_its_count():
    LY, FT = sub("layout"), sub("finetune")
    pe = [LY.Entry(f"p{j}", (8,), "ones", True, offset=8 * j) for j in range(1100)]
    with pytest.raises(ValueError, match="1100"):
        FT.ParamGroups(pe, [_P() for _ in pe], [{"params": [e.name for e in pe[::2]]}])       # alternating groups: no merge at all
    FT.ParamGroups(pe[:512], [_P() for _ in pe[:512]], [{"params": [e.name for e in pe[:512:2]]}])   # 512 rows fit


# ------------------------------------------------------------------------------------------------------- no_weight_decay_groups
def test_no_weight_decay_groups_partition_by_dimension():
    FT = sub("finetune")
    m = pkg().load_dropin().VQAModel(**CFG, compute_dtype="fp32")
    flat, rest = FT.no_weight_decay_groups(m, lr_scale=0.5)
    assert flat["weight_decay"] == 0.0 and rest["weight_decay"] is None and flat["lr_scale"] == rest["lr_scale"] == 0.5
    names = [e.name for e in m._param_entries]
    assert sorted(flat["params"] + rest["params"]) == sorted(names) and not set(flat["params"]) & set(rest["params"])
    shape = {e.name: e.shape for e in m._param_entries}
    for n in names:
        one_d = (n.endswith(".bias") or re.search(r"\.bn\d\.weight$", n) or re.search(r"\.norm\w*\.weight$", n) or ".final_norm." in n)
        if one_d:
            assert n in flat["params"], n
        if n == "fusion.image_projector.position_embedding" or (n.endswith(".weight") and len(shape[n]) >= 2):
            assert n in rest["params"], n                               # conv, linear and embedding weights
    assert "text_encoder.token_embedding.weight" in rest["params"] and "image_encoder.stem.0.weight" in rest["params"]
    assert "image_encoder.stem.1.weight" in flat["params"] and "fusion.output_norm.weight" in flat["params"]
    assert all(len(shape[n]) <= 1 for n in flat["params"]) and all(len(shape[n]) > 1 for n in rest["params"])
    assert FT.no_weight_decay_groups(m)[0]["lr_scale"] == 1.0
    pg = FT.ParamGroups(m._param_entries, m._param_list(), [flat, rest])
    assert len(pg.groups) == 2                                          # a partition: no implicit group


# ---------------------------------------------------------------------------------------------- the range table under groups
def test_group_boundaries_split_ranges_and_nothing_else_changes():
    FT = sub("finetune")
    pe = _entries()
    n = len(pe)
    every = (True,) * n
    # a group boundary splits a merge
    grp = [0] * n
    grp[5] = 1
    r = FT.trainable_ranges(pe, every, None, grp)
    assert [x[2] for x in r] == [0, 5, 6] and r[1][:2] == (pe[5].offset, FT.slot_end(pe[5]))
    assert sum(hi - lo for lo, hi, _ in r) == FT.slot_end(pe[-1]) - pe[0].offset
    # equal group and equal lag still merge -- whatever the group's number
    assert FT.trainable_ranges(pe, every, [0] * n, [3] * n) == FT.trainable_ranges(pe, every)
    assert len(FT.trainable_ranges(pe, every, [0] * n, [3] * n)) == 1
    # lag and group boundaries both split
    lag = [0] * n
    lag[2] = 1
    assert [x[2] for x in FT.trainable_ranges(pe, every, lag, grp)] == [0, 2, 3, 5, 6]
    # frozen parameters still interrupt, and a group boundary beside one adds nothing
    tr = tuple(j != 5 for j in range(n))
    assert FT.trainable_ranges(pe, tr, None, grp) == FT.trainable_ranges(pe, tr)
    # without the group argument: today's output (restated here), for a few masks and lag classes
    def today(trainable, lag_class=None):
        out, prev = [], None
        for j, (e, t) in enumerate(zip(pe, trainable)):
            if not t:
                prev = None
                continue
            cls = 0 if lag_class is None else lag_class[j]
            if prev is not None and out and out[-1][1] == e.offset and prev == cls:
                out[-1][1] = FT.slot_end(e)
            else:
                out.append([e.offset, FT.slot_end(e), j])
            prev = cls
        return [tuple(x) for x in out]
    for mask in (every, tuple(j % 3 != 0 for j in range(n)), tuple(not e.name.startswith("image_encoder.") for e in pe)):
        for lc in (None, lag, [j % 2 for j in range(n)]):
            got = FT.trainable_ranges(pe, mask, lc)
            assert got == today(mask, lc) and all(len(x) == 3 for x in got)
    # range_table_rows is unchanged: {lo, hi, pos, lag index}
    assert FT.range_table_rows(r) == [[r[0][0], r[0][1], 0, 0], [r[1][0], r[1][1], r[0][1] - r[0][0], 5],
                                      [r[2][0], r[2][1], r[1][1] - r[0][0], 6]]


@pytest.mark.parametrize("cfg,rows,rows_backbone", [(O.full_config(), 86, 87),
                                                    (O.full_config(num_transformer_layers=8, embed_dim=512, num_answers=2000), 110, 111)])
def test_row_counts_under_no_weight_decay_groups(cfg, rows, rows_backbone):
    """default and stress config: the table the no-decay recipe needs, alone and composed with a backbone rate, fits 512 rows"""
    FT = sub("finetune")
    pe = _entries(cfg)

    class M:
        _param_entries = pe
    groups = FT.no_weight_decay_groups(M)
    pg = _resolve(groups, pe)
    r = FT.trainable_ranges(pe, (True,) * len(pe), None, pg.group_of)
    assert len(r) == rows <= 512
    split = []
    for g in groups:                                                    # split by the prefix first
        cnn = [n for n in g["params"] if n.startswith("image_encoder.")]
        split += [dict(g, params=cnn, lr_scale=0.1), dict(g, params=[n for n in g["params"] if n not in set(cnn)])]
    pg = _resolve(split, pe)
    assert len(pg.groups) == 4
    assert len(FT.trainable_ranges(pe, (True,) * len(pe), None, pg.group_of)) == rows_backbone <= 512


# ------------------------------------------------------------------------------------------------------------------ the block
@pytest.mark.parametrize("rel", ["include/vqa_hip.h", "visual-question-answering-vqa-system_amd/csrc/common.h"])
def test_ctypes_view_of_the_group_block(rel):
    SG, FT = sub("stepgraph"), sub("finetune")
    assert ctypes.sizeof(SG.GroupHyper) == SG.GROUP_HYPER_BYTES == 128
    assert SG.GroupHyper.lr_scale.offset == 0 and SG.GroupHyper.wd.offset == 64
    assert SG.GROUPS_MAX == FT.GROUPS_MAX == 16 and FT.RANGES_MAX == 512
    txt = open(os.path.join(REPO, *rel.split("/"))).read()
    if rel.endswith("common.h"):                 # the sources compile the header's block itself: common.h includes it and pins its layout
        assert re.search(r'^#include "\.\./\.\./include/vqa_hip\.h"', txt, flags=re.M)
        assert "static_assert(sizeof(vqa_group_hyper) == 128 && alignof(vqa_group_hyper) == 16 && offsetof(vqa_group_hyper, wd) == 64" in txt
        return
    assert re.search(r"#define VQA_GROUPS_MAX 16\b", txt)
    m = re.search(r"typedef struct __attribute__\(\(aligned\(16\)\)\) vqa_group_hyper \{(.*?)\} vqa_group_hyper;", txt, flags=re.S)
    assert m and [d.strip() for d in m.group(1).split(";") if d.strip()] == ["float lr_scale[VQA_GROUPS_MAX]", "float wd[VQA_GROUPS_MAX]"]


def test_the_new_entries_are_declared_and_bound():
    L = sub("_lib")
    S, P, I = L.SIGNATURES, L.P, L.I
    assert S["vqa_group_hyper_set"] == [P, I, P, P, P]
    for sfx in ("", "_ema", "_dev", "_ema_dev"):                        # the range entry's arguments + group_of_range, groups
        assert S["vqa_adamw_groups" + sfx] == S["vqa_adamw_ranges" + sfx][:-1] + [P, P, P]
    txt = open(os.path.join(REPO, "include", "vqa_hip.h")).read()
    for name in ("vqa_group_hyper_set", "vqa_adamw_groups", "vqa_adamw_groups_ema", "vqa_adamw_groups_dev", "vqa_adamw_groups_ema_dev"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), name


# -------------------------------------------------------------------------------------------------------------------- the key
def test_step_key_sees_the_structure_of_the_groups_and_not_their_values():
    SG = sub("stepgraph")
    pe = _entries()

    def key(groups):
        return SG.step_key(features=False, images=torch.zeros(4, 3, 8, 8), token_ids=torch.zeros(4, 10, dtype=torch.long), attention_mask=None,
                           image_index=None, targets=torch.zeros(4, dtype=torch.long), plan=None, loss_kind="ce", loss_opts=(0.0, None, None),
                           ema=False, metrics=None, flat_ptr=0x1000, wsrc_ptr=0x2000, table_id=SG.table_id(1, groups))

    a = _resolve([{"params": ["image_encoder."], "lr_scale": 0.1}], pe)
    b = _resolve([{"params": ["image_encoder."], "lr_scale": 0.5, "weight_decay": 0.0}], pe)      # other values, same structure
    c = _resolve([{"params": ["text_encoder."], "lr_scale": 0.1}], pe)                             # another structure
    assert key(a.key()) == key(b.key())
    b.groups[0]["lr_scale"] = 3.0
    assert key(a.key()) == key(b.key())
    assert key(a.key()) != key(None) and key(a.key()) != key(c.key())
    neutral = _resolve([{"params": [e.name for e in pe]}], pe)          # one group over everything is still a grouped step
    assert key(neutral.key()) != key(None)
    # without the argument the key is what it was
    plain = SG.step_key(features=False, images=torch.zeros(4, 3, 8, 8), token_ids=torch.zeros(4, 10, dtype=torch.long), attention_mask=None,
                        image_index=None, targets=torch.zeros(4, dtype=torch.long), plan=None, loss_kind="ce", loss_opts=(0.0, None, None),
                        ema=False, metrics=None, flat_ptr=0x1000, wsrc_ptr=0x2000, table_id=1)
    assert plain == key(None) and len(plain) == 14 and SG.table_id(None) is None and SG.table_id(7) == 7


def test_trainer_constructor_refuses_bad_groups_before_anything_else(monkeypatch):
    """the refusals come ahead of the engine: nothing is allocated (no GPU here, so reaching the engine would fail differently)"""
    TR = sub("trainer")
    m = pkg().load_dropin().VQAModel(**CFG, compute_dtype="fp32")
    monkeypatch.setattr(type(m), "_ensure_engine", lambda self: (_ for _ in ()).throw(AssertionError("the engine was reached")))
    with pytest.raises(KeyError):
        TR.HipTrainer(m, param_groups=[{"params": ["nope."]}])
    with pytest.raises(ValueError):
        TR.HipTrainer(m, param_groups=[{"params": ["fusion."]}, {"params": ["fusion.output_norm.weight"]}])
    with pytest.raises(ValueError):
        TR.HipTrainer(m, param_groups=[{"params": []}])
    with pytest.raises(ValueError):
        TR.HipTrainer(m, param_groups=[{"params": ["fusion."], "lr_scale": -1.0}])
    with pytest.raises(AssertionError, match="engine"):                 # good groups pass the host checks
        TR.HipTrainer(m, param_groups=sub("finetune").no_weight_decay_groups(m))
