"""CPU: the many-questions-per-image surface exists end to end -- the two indexed attention entries are declared, bound with the
header's arity and exported by the built library, and the drop-in exposes encode_images / answer and image_index on forward,
predict and get_attention_maps (no GPU: nothing is launched)."""
import ctypes
import inspect
import os
import re

from _pkg import REPO, pkg, sub

NEW = ("vqa_attention_fwd_idx", "vqa_attention_fwd_mfma_idx")


def _header_decls():
    txt = open(os.path.join(REPO, "include", "vqa_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return {m.group(1): len([a for a in m.group(2).split(",") if a.strip()])
            for m in re.finditer(r"\bint\s+(vqa_\w+)\s*\((.*?)\)\s*;", txt, flags=re.S)}


def test_header_declares_the_indexed_entries_with_the_table_arity():
    decls, L = _header_decls(), sub("_lib")
    for name in NEW:
        assert name in decls, name
        assert name in L.SIGNATURES, name
        assert decls[name] == len(L.SIGNATURES[name]), (name, decls[name], len(L.SIGNATURES[name]))
    # kv_index (int*) and n_kv follow the three strides; the mfma form is the generic one minus dtype
    assert L.SIGNATURES["vqa_attention_fwd_idx"][1:] == L.SIGNATURES["vqa_attention_fwd_mfma_idx"]
    assert L.SIGNATURES["vqa_attention_fwd_mfma_idx"][6:8] == [ctypes.c_void_p, ctypes.c_int]


def test_library_exports_the_indexed_entries():
    import __graft_entry__ as G
    G.build()
    lib = ctypes.CDLL(sub("_lib").LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name


def test_indexed_entries_reject_bad_arguments_before_any_hip_call():
    """Argument errors (status 1000) are returned before the entry touches the runtime, so this runs without a GPU."""
    import __graft_entry__ as G
    G.build()
    lib = sub("_lib").lib()
    mfma, valu = lib.vqa_attention_fwd_mfma_idx, lib.vqa_attention_fwd_idx
    # NULL index, negative image count, head dim outside {32, 64}, a row stride that is not a multiple of 8
    assert mfma(1, 1, 1, 256, 512, 512, None, 2, None, 1, 1, 256, 2, 8, 20, 49, 32, None) == 1000
    assert mfma(1, 1, 1, 256, 512, 512, 1, -1, None, 1, 1, 256, 2, 8, 20, 49, 32, None) == 1000
    assert mfma(1, 1, 1, 256, 512, 512, 1, 2, None, 1, 1, 256, 2, 8, 20, 49, 48, None) == 1000
    assert mfma(1, 1, 1, 256, 516, 512, 1, 2, None, 1, 1, 256, 2, 8, 20, 49, 32, None) == 1000
    assert valu(1, 1, 1, 1, 256, 512, 512, None, 2, None, 1, 1, 256, 2, 8, 20, 49, 32, None) == 1000
    assert valu(1, 1, 1, 1, 256, 512, 512, 1, -3, None, 1, 1, 256, 2, 8, 20, 49, 32, None) == 1000


def test_dropin_exposes_the_multi_question_api():
    M = pkg().load_dropin()
    V = M.VQAModel
    assert callable(getattr(V, "encode_images", None)) and callable(getattr(V, "answer", None))
    for meth in ("forward", "predict", "get_attention_maps"):
        params = inspect.signature(getattr(V, meth)).parameters
        assert "image_index" in params and params["image_index"].default is None, meth
    ap = inspect.signature(V.answer).parameters
    assert list(ap)[:3] == ["self", "context", "token_ids"]
    assert ap["attention_mask"].default is None and ap["image_index"].default is None and ap["return_aux"].default is False


def test_engine_splits_the_eval_forward():
    E = sub("engine").HipEngine
    assert callable(getattr(E, "encode_images", None)) and callable(getattr(E, "answer", None))
    p = inspect.signature(E._attn_block_fwd).parameters
    assert p["kv_index"].default is None


def test_cpu_model_refuses_the_new_paths_without_launching():
    import pytest
    import torch
    M = pkg().load_dropin()
    m = M.VQAModel(compute_dtype="fp32", seed=0).eval()
    x, ids = torch.zeros(2, 3, 224, 224), torch.ones(3, 20, dtype=torch.long)
    with torch.no_grad():
        with pytest.raises(RuntimeError):            # no CPU path, index or not
            m(x, ids, image_index=torch.tensor([0, 1, 1]))
        with pytest.raises(RuntimeError):
            m.encode_images(x)
