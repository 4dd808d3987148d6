"""CPU: the many-questions-per-image TRAINING surface exists end to end -- the CSR builder, the dropout forwards and the indexed
backwards are declared with the table's arity and exported by the built library, their argument errors come back as 1000 before
any HIP call, the drop-in exposes forward_grouped / group_by_image and HipTrainer.step takes image_index (no GPU: nothing is
launched)."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from _pkg import REPO, pkg, sub

NEW = ("vqa_index_csr", "vqa_attention_fwd_idx_train", "vqa_attention_fwd_mfma_idx_train", "vqa_attention_bwd_idx",
       "vqa_attention_bwd_mfma_idx")


def _header_decls():
    txt = open(os.path.join(REPO, "include", "vqa_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return {m.group(1): len([a for a in m.group(2).split(",") if a.strip()])
            for m in re.finditer(r"\bint\s+(vqa_\w+)\s*\((.*?)\)\s*;", txt, flags=re.S)}


def test_header_declares_the_new_entries_with_the_table_arity():
    decls, L = _header_decls(), sub("_lib")
    for name in NEW:
        assert name in decls, name
        assert name in L.SIGNATURES, name
        assert decls[name] == len(L.SIGNATURES[name]), (name, decls[name], len(L.SIGNATURES[name]))
    S = L.SIGNATURES
    # the _train forwards are the indexed forwards plus (p, seed); the mfma forms are the generic ones minus dtype
    assert S["vqa_attention_fwd_idx_train"] == S["vqa_attention_fwd_idx"][:-1] + [ctypes.c_float, ctypes.c_ulonglong, ctypes.c_void_p]
    assert S["vqa_attention_fwd_idx_train"][1:] == S["vqa_attention_fwd_mfma_idx_train"]
    assert S["vqa_attention_bwd_idx"][1:] == S["vqa_attention_bwd_mfma_idx"]
    # the indexed backward is vqa_attention_bwd with (offsets, order, n_kv) after probs
    assert S["vqa_attention_bwd_idx"][:10] + S["vqa_attention_bwd_idx"][13:] == S["vqa_attention_bwd"]


def test_library_exports_the_new_entries():
    import __graft_entry__ as G
    G.build()
    lib = ctypes.CDLL(sub("_lib").LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name


def test_new_entries_reject_bad_arguments_before_any_hip_call():
    import __graft_entry__ as G
    G.build()
    lib = sub("_lib").lib()
    # vqa_index_csr: negative sizes, NULL outputs, too many images
    assert lib.vqa_index_csr(1, -1, 4, 1, 1, None) == 1000
    assert lib.vqa_index_csr(1, 4, -1, 1, 1, None) == 1000
    assert lib.vqa_index_csr(1, 4, 4, None, 1, None) == 1000
    assert lib.vqa_index_csr(None, 4, 4, 1, 1, None) == 1000
    assert lib.vqa_index_csr(1, 4, 1 << 20, 1, 1, None) == 1000
    # _train forwards: NULL index, negative image count, dropout outside [0, 1), head dim outside {32, 64}
    ft, fm = lib.vqa_attention_fwd_idx_train, lib.vqa_attention_fwd_mfma_idx_train
    assert ft(1, 1, 1, 1, 256, 512, 512, None, 2, None, 1, 1, 256, 2, 8, 20, 49, 32, 0.1, 1, None) == 1000
    assert ft(1, 1, 1, 1, 256, 512, 512, 1, -1, None, 1, 1, 256, 2, 8, 20, 49, 32, 0.1, 1, None) == 1000
    assert ft(1, 1, 1, 1, 256, 512, 512, 1, 2, None, 1, 1, 256, 2, 8, 20, 49, 32, 1.0, 1, None) == 1000
    assert fm(1, 1, 1, 256, 512, 512, 1, 2, None, 1, 1, 256, 2, 8, 20, 49, 48, 0.1, 1, None) == 1000
    assert fm(1, 1, 1, 256, 512, 512, None, 2, None, 1, 1, 256, 2, 8, 20, 49, 32, 0.1, 1, None) == 1000
    # indexed backwards: NULL offsets, negative image count, Lk beyond the MFMA tiles, a row stride that is not a multiple of 8
    bv, bm = lib.vqa_attention_bwd_idx, lib.vqa_attention_bwd_mfma_idx
    a = (1, 256, 1, 1, 1, 256, 512, 512, 1)
    tail = (1, 1, 1, 256, 512, 512, 6, 8, 20, 49, 32, 0.1, 1, None)
    assert bv(1, *a, None, 1, 3, *tail) == 1000
    assert bv(1, *a, 1, 1, -1, *tail) == 1000
    assert bv(1, *a, 1, 1, 3, 1, 1, 1, 256, 512, 512, 6, 8, 20, 49, 320, 0.1, 1, None) == 1000     # Lk * hd too large
    assert bm(*a, None, 1, 3, *tail) == 1000
    assert bm(*a, 1, 1, 3, 1, 1, 1, 256, 512, 512, 6, 8, 20, 161, 32, 0.1, 1, None) == 1000
    assert bm(1, 256, 1, 1, 1, 260, 512, 512, 1, 1, 1, 3, *tail) == 1000


def test_dropin_and_trainer_signatures():
    M = pkg().load_dropin()
    fp = inspect.signature(M.VQAModel.forward_grouped).parameters
    assert list(fp) == ["self", "images", "token_ids", "attention_mask", "image_index", "return_aux"]
    assert fp["attention_mask"].default is None and fp["image_index"].default is None and fp["return_aux"].default is False
    sp = inspect.signature(sub("trainer").HipTrainer.step).parameters
    assert list(sp) == ["self", "images", "token_ids", "attention_mask", "targets", "metrics", "image_index"]
    assert sp["metrics"].default is None and sp["image_index"].default is None
    assert inspect.signature(sub("engine").HipEngine.forward).parameters["kv_index"].default is None
    assert callable(M.group_by_image)


def test_cpu_model_refuses_forward_grouped():
    M = pkg().load_dropin()
    m = M.VQAModel(compute_dtype="fp32", seed=0).train()
    x, ids = torch.zeros(2, 3, 224, 224), torch.ones(3, 20, dtype=torch.long)
    with pytest.raises(RuntimeError):
        m.forward_grouped(x, ids, image_index=torch.tensor([0, 1, 1]))
    m.eval()
    with torch.no_grad(), pytest.raises(RuntimeError):
        m.forward_grouped(x, ids, image_index=torch.tensor([0, 1, 1]))


@pytest.mark.parametrize("ids, first, index", [
    ([7, 7, 3, 9, 3, 7], [0, 2, 3], [0, 0, 1, 2, 1, 0]),
    ([5, 6, 7], [0, 1, 2], [0, 1, 2]),
    ([4, 4, 4, 4], [0], [0, 0, 0, 0]),
    ([], [], []),
    ([139, 285, 139, 632, 285, 632, 724], [0, 1, 3, 6], [0, 1, 0, 2, 1, 2, 3]),
])
def test_group_by_image(ids, first, index):
    M = pkg().load_dropin()
    for arg in (ids, torch.tensor(ids, dtype=torch.long)):
        f, i = M.group_by_image(arg)
        assert f.dtype == torch.long and i.dtype == torch.long
        assert f.tolist() == first and i.tolist() == index
        if ids:                                                   # images[first][index] reproduces the batch's image ids
            t = torch.tensor(ids)
            assert torch.equal(t[f][i], t)
