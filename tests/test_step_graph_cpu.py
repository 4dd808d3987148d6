"""CPU: the host logic of the captured train step (stepgraph.py) -- the self-describing seed word against a Python model of
drop_resolve (csrc/common.h), the ctypes view of vqa_step_state against include/vqa_hip.h, and the key a captured graph is filed
under.  Nothing here needs the library or a GPU."""
import ctypes
import os
import re
from collections import namedtuple

import pytest
import torch

from _pkg import REPO, sub

SG = sub("stepgraph")
SoftTargets = namedtuple("SoftTargets", "ids weights counts")


# ------------------------------------------------------------------------------------------------------------------ seed words
def test_seed_word_round_trip_and_resolution():
    memory = {}
    for addr in (8, 0x7F12_3456_7808, (1 << 48) - 8):
        for site in (0, 1, 37, 4095):
            w = SG.seed_word(addr, site)
            assert SG.is_indirect(w) and w < (1 << 64) and SG.decode_seed_word(w) == (addr, site)
            for rank, step in ((0, 1), (7, 123456), (1023, 0xFFFFFFFF - 0x5EED)):
                memory[addr] = SG.seed_step(rank, 0x5EED, step)
                assert memory[addr] & 0xFFF == 0
                assert SG.resolve(w, memory.__getitem__) == SG.plain_seed(rank, 0x5EED, step, site)
    # a plain seed resolves to itself and nothing is read
    def no_read(addr):
        raise AssertionError("a plain seed reads nothing")
    s = SG.plain_seed(5, 0x5EED, 99, 17)
    assert SG.resolve(s, no_read) == s
    with pytest.raises(ValueError):
        SG.decode_seed_word(s)


def test_seed_word_refuses_what_does_not_fit():
    for addr in (0, 1 << 48, (1 << 48) + 8, 12):                 # NULL, beyond 48 bits, not 8-byte aligned
        with pytest.raises(ValueError):
            SG.seed_word(addr, 1)
    for site in (-1, 4096):
        with pytest.raises(ValueError):
            SG.seed_word(0x1000, site)


def test_plain_seeds_of_the_existing_format_never_carry_the_flag():
    # rank << 44 | step << 12 | site: the step field is 32 bits wide (bits 12-43); bit 63 needs a rank of 2^19 or more
    for rank in (0, 1, 7, 1023, (1 << 19) - 1):
        for step in (0, 1, 0xFFFFFFFF, 1 << 40):
            for site in (0, 1, 4095):
                s = SG.plain_seed(rank, 0x5EED, step, site)
                assert not SG.is_indirect(s)
                assert s == (rank << 44) | (((0x5EED + step) & 0xFFFFFFFF) << 12) | site           # HipEngine._seed()'s expression
    assert SG.is_indirect(SG.plain_seed(1 << 19, 0x5EED, 0, 0))   # where the format would end: half a million ranks


def test_engine_hands_out_the_flagged_form_while_a_source_is_set():
    E = sub("engine").HipEngine
    eng = E.__new__(E)
    eng.seed_rank, eng.seed_base, eng.step_id, eng._site, eng._seed_src = 2, 0x5EED, 41, 0, None
    assert eng._seed() == SG.plain_seed(2, 0x5EED, 41, 1)
    eng._seed_src = 0x7F00_0000_1008
    w = eng._seed()
    assert SG.decode_seed_word(w) == (0x7F00_0000_1008, 2)
    assert SG.resolve(w, {0x7F00_0000_1008: SG.seed_step(2, 0x5EED, 41)}.__getitem__) == SG.plain_seed(2, 0x5EED, 41, 2)
    eng._seed_src = None
    assert eng._seed() == SG.plain_seed(2, 0x5EED, 41, 3)


# ------------------------------------------------------------------------------------------------------------- the state block
CTYPES = {"long long": ctypes.c_longlong, "unsigned long long": ctypes.c_ulonglong, "float": ctypes.c_float, "int": ctypes.c_int}


def _header_fields(rel):
    txt = open(os.path.join(REPO, *rel.split("/"))).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    txt = re.sub(r"//[^\n]*", "", txt)
    m = re.search(r"typedef struct __attribute__\(\(aligned\((\d+)\)\)\) vqa_step_state \{(.*?)\} vqa_step_state;", txt, flags=re.S)
    assert m, rel
    fields = []
    for decl in m.group(2).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ = next(t for t in sorted(CTYPES, key=len, reverse=True) if decl.startswith(t + " "))
        fields += [(name.strip(), CTYPES[typ]) for name in decl[len(typ):].split(",")]
    return int(m.group(1)), fields


@pytest.mark.parametrize("rel", ["include/vqa_hip.h", "visual-question-answering-vqa-system_amd/csrc/common.h"])
def test_ctypes_structure_matches_the_declared_struct(rel):
    if rel.endswith("common.h"):                 # the sources compile the header's struct itself: common.h includes it and pins its layout
        txt = open(os.path.join(REPO, *rel.split("/"))).read()
        assert re.search(r'^#include "\.\./\.\./include/vqa_hip\.h"', txt, flags=re.M)
        assert "static_assert(sizeof(vqa_step_state) == 64 && alignof(vqa_step_state) == 16" in txt
        assert ("static_assert(offsetof(vqa_step_state, seed_step) == 8 && offsetof(vqa_step_state, lr) == 16 && "
                "offsetof(vqa_step_state, ema_warmup) == 48") in txt
        return
    align, fields = _header_fields(rel)
    mine = [(n, t) for n, t in SG.StepState._fields_ if n != "_pad"]
    assert mine == fields
    assert [n for n, _ in fields] == ["calls", "seed_step", "lr", "b1", "b2", "eps", "wd", "max_norm", "gscale", "ema_decay", "ema_warmup"]

    class Packed(ctypes.Structure):                             # the C layout of those fields, rounded up to the declared alignment
        _fields_ = fields
    size = (ctypes.sizeof(Packed) + align - 1) // align * align
    assert align == 16 and size == ctypes.sizeof(SG.StepState) == SG.STATE_BYTES == 64
    for n, _ in fields:
        assert getattr(SG.StepState, n).offset == getattr(Packed, n).offset
    assert SG.StepState.seed_step.offset == SG.SEED_STEP_OFFSET == 8


# --------------------------------------------------------------------------------------------------------------------- the key
Plan = namedtuple("Plan", "trainable modes")


def _key(**over):
    B, L = 4, 10
    kw = dict(features=True, images=torch.zeros(B, 2, 2, 512, dtype=torch.bfloat16), token_ids=torch.zeros(B, L, dtype=torch.long),
              attention_mask=torch.zeros(B, L), image_index=None, targets=torch.zeros(B, dtype=torch.long),
              plan=Plan((False, True, True), (False, True, True, True)), loss_kind="ce", loss_opts=(0.0, None, None), ema=True, metrics=None,
              flat_ptr=0x1000, wsrc_ptr=0x2000, table_id=1)
    kw.update(over)
    return SG.step_key(**kw)


def test_key_changes_with_what_decides_the_launches():
    base = _key()
    m1, m2 = object(), object()
    soft = SoftTargets(torch.zeros(4, 2, dtype=torch.int32), torch.zeros(4, 2), None)
    changes = dict(
        batch=dict(images=torch.zeros(5, 2, 2, 512, dtype=torch.bfloat16)),
        length=dict(token_ids=torch.zeros(4, 12, dtype=torch.long), attention_mask=torch.zeros(4, 12)),
        dtype=dict(images=torch.zeros(4, 2, 2, 512)),
        no_mask=dict(attention_mask=None),
        index=dict(image_index=torch.zeros(4, dtype=torch.int32)),
        route=dict(features=False),
        soft=dict(targets=soft),
        soft_k=dict(targets=SoftTargets(torch.zeros(4, 3, dtype=torch.int32), torch.zeros(4, 3), None)),
        soft_counts=dict(targets=SoftTargets(soft.ids, soft.weights, torch.zeros(4, 2, dtype=torch.int32))),
        trainable=dict(plan=Plan((False, False, True), (False, True, True, True))),
        modes=dict(plan=Plan((False, True, True), (False, False, True, True))),
        no_plan=dict(plan=None),
        loss_kind=dict(loss_kind="bce"),
        loss_opts=dict(loss_opts=(0.1, -100, None)),
        ema_off=dict(ema=False),
        metrics=dict(metrics=m1),
        flat=dict(flat_ptr=0x3000),
        wsrc=dict(wsrc_ptr=0x4000),
        table=dict(table_id=2),
        no_table=dict(table_id=None),
    )
    keys = {name: _key(**kw) for name, kw in changes.items()}
    for name, k in keys.items():
        assert k != base, name
        hash(k)
    assert len(set(keys.values())) == len(keys)
    assert _key(metrics=m1) == _key(metrics=m1) != _key(metrics=m2)            # identity, not equality or type


def test_key_ignores_values():
    base = _key()
    B, L = 4, 10
    same = dict(
        images=dict(images=torch.ones(B, 2, 2, 512, dtype=torch.bfloat16)),
        ids=dict(token_ids=torch.full((B, L), 7, dtype=torch.long)),
        mask=dict(attention_mask=torch.ones(B, L)),
        targets=dict(targets=torch.arange(B)),
    )
    for name, kw in same.items():
        assert _key(**kw) == base, name
    idx = dict(image_index=torch.zeros(B, dtype=torch.int32))
    assert _key(**idx) == _key(image_index=torch.ones(B, dtype=torch.int32))
    s = lambda v: SoftTargets(torch.full((B, 2), v, dtype=torch.int32), torch.full((B, 2), float(v)), None)
    assert _key(targets=s(1)) == _key(targets=s(2))
    # lr, betas, eps, weight decay, max_norm, the EMA decay and warm-up flag and the step number are no arguments of the key at all:
    # they reach a captured step through the device state block
    import inspect
    assert set(inspect.signature(SG.step_key).parameters) == {"features", "images", "token_ids", "attention_mask", "image_index", "targets",
                                                              "plan", "loss_kind", "loss_opts", "ema", "metrics", "flat_ptr", "wsrc_ptr",
                                                              "table_id"}
