"""CPU: tests/_arena.py sees what it claims to see, and every pointer-taking entry of the GEMM / conv / stem sources has an arena case.

The first half plants the faults the GPU module (tests/test_gpu_arena_gemm_conv.py) exists to catch -- a byte changed in a moat, an
input payload modified, an output element left unwritten, a read one row before an operand -- into a device="cpu" Arena and asserts
that check() (or the NaN) reports each one.  The second half is the completeness guard: the entries come from include/vqa_hip.h."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import _arena as A
from _pkg import REPO, sub

BF, F32 = torch.bfloat16, torch.float32
SOURCES = ["gemm_conv.hip", "gemm8p.hip", "conv_c64.hip", "stem_conv.hip", "stem_dgrad.hip", "mxfp8.hip"]
CSRC = os.path.join(REPO, "visual-question-answering-vqa-system_amd", "csrc")


def _every_kind(ar):
    """one operand of each kind; returns {kind name: tensor}"""
    g = torch.Generator().manual_seed(3)
    return {
        "put_bf16": ar.put(torch.randint(-8, 9, (5, 24), generator=g).double(), BF, name="put_bf16"),
        "put_f32": ar.put(torch.randint(-8, 9, (7, 3), generator=g).double(), F32, name="put_f32"),
        "put_u8": ar.put(torch.randint(0, 255, (2, 5, 7, 3), generator=g, dtype=torch.int64).to(torch.uint8), name="put_u8"),
        "out_bf16": ar.out((9, 10), BF, name="out_bf16"),
        "out_f32": ar.out((3, 5), F32, name="out_f32"),
        "out_u8": ar.out((33,), torch.uint8, name="out_u8"),
        "acc_f32": ar.acc(torch.arange(12.0).view(3, 4), F32, name="acc_f32"),
        "acc_i64": ar.acc(torch.zeros(17, dtype=torch.int64), name="acc_i64"),
        "scratch": ar.scratch(21, name="scratch"),
    }


def _write_outputs(ops):
    for k, t in ops.items():
        if k.startswith("out_"):
            t.copy_(torch.ones(t.shape).to(t.dtype))


KINDS = ["put_bf16", "put_f32", "put_u8", "out_bf16", "out_f32", "out_u8", "acc_f32", "acc_i64", "scratch"]


def test_clean_arena_passes_and_free_payloads_may_change():
    ar = A.Arena("cpu")
    ops = _every_kind(ar)
    _write_outputs(ops)
    ops["acc_f32"].add_(3)
    ops["acc_i64"].add_(1)
    ops["scratch"].zero_()
    ar.check()


@pytest.mark.parametrize("side", ["low", "high"])
@pytest.mark.parametrize("where", ["adjacent", "far"])
@pytest.mark.parametrize("kind", KINDS)
def test_one_changed_moat_byte_of_any_operand_kind_fails(kind, side, where):
    ar = A.Arena("cpu")
    ops = _every_kind(ar)
    _write_outputs(ops)
    op = ar.operand(ops[kind])
    if side == "low":
        i = op.lo - 1 if where == "adjacent" else 0
    else:
        i = op.lo + op.nbytes if where == "adjacent" else op.buf.numel() - 1
    op.buf[i] ^= 1
    with pytest.raises(AssertionError, match=rf"{kind}: {side} moat changed at byte "):
        ar.check()


def test_moat_failure_names_the_offset():
    ar = A.Arena("cpu")
    t = ar.put(torch.zeros(8), F32, name="x")
    op = ar.operand(t)
    op.buf[op.lo - 4096] = 0
    with pytest.raises(AssertionError, match=r"x: low moat changed at byte -4096 relative"):
        ar.check()
    op.buf[op.lo - 4096] = op.image[op.lo - 4096]
    op.buf[op.lo + op.nbytes + 7] = 0
    with pytest.raises(AssertionError, match=r"x: high moat changed at byte 7 past"):
        ar.check()


@pytest.mark.parametrize("kind", ["put_bf16", "put_f32", "put_u8"])
def test_changed_input_payload_fails(kind):
    ar = A.Arena("cpu")
    ops = _every_kind(ar)
    _write_outputs(ops)
    op = ar.operand(ops[kind])
    op.buf[op.lo + 5] ^= 0x10
    with pytest.raises(AssertionError, match=rf"{kind}: input payload changed at byte 5 "):
        ar.check()


@pytest.mark.parametrize("kind", ["out_bf16", "out_f32", "out_u8"])
def test_untouched_output_element_fails_unless_the_case_marks_it(kind):
    ar = A.Arena("cpu")
    ops = _every_kind(ar)
    _write_outputs(ops)
    op = ar.operand(ops[kind])
    flat = ops[kind].view(-1)
    es = flat.element_size()
    flat.view(torch.uint8)[2 * es: 3 * es] = op.image[op.lo + 2 * es: op.lo + 3 * es]          # element 2 never written
    with pytest.raises(AssertionError, match=rf"{kind}: out payload not overwritten: 1 of \d+ elements .* first at byte {2 * es}"):
        ar.check()
    stay = torch.zeros(flat.numel(), dtype=torch.bool)
    stay[2] = True
    op.may_stay = stay.view(ops[kind].shape)
    ar.check()


def test_fill_word_is_nan_in_both_float_views():
    w = torch.tensor([A.FILL_WORD], dtype=torch.int32)
    assert bool(torch.isnan(w.view(F32)).all())
    assert bool(torch.isnan(w.view(BF).float()).all()) and w.view(BF).numel() == 2
    ar = A.Arena("cpu")
    for dtype in (BF, F32):
        o = ar.out((6, 5), dtype)
        assert bool(torch.isnan(o.float()).all())
        assert bool(torch.isnan(ar.scratch(9)).all())
    assert bool((ar.out((5,), torch.uint8) == A.FILL_BYTE).all())


def test_payload_addresses_have_the_promised_skew():
    assert A.SKEW == 16 == sub("layout").ALIGN * 2 and A.MOAT == 65536 and A.MOAT % A.BOUNDARY == 0
    ar = A.Arena("cpu")
    ops = _every_kind(ar)
    for k, t in ops.items():
        op = ar.operand(t)
        assert t.data_ptr() - op.buf.data_ptr() == A.MOAT + A.SKEW, k
        assert (t.data_ptr() - op.buf.data_ptr()) % A.BOUNDARY == 16, k
        assert op.buf.numel() - (op.lo + op.nbytes) >= A.MOAT, k
    strict = ar.put(torch.zeros(4), F32, skew=0)
    assert (strict.data_ptr() - ar.operand(strict).buf.data_ptr()) % A.BOUNDARY == 0


def test_put_keeps_the_bits_and_acc_the_values():
    ar = A.Arena("cpu")
    src = torch.randint(-8, 9, (4, 6)).double()
    assert torch.equal(ar.put(src, BF), src.to(BF)) and torch.equal(ar.acc(src, F32), src.float())


def test_convolution_over_a_view_with_one_moat_row_is_nan():
    """the reference convolution of an activation read one image row early: the row of moat NaNs reaches the output (weights of zero
    included: 0 x NaN is NaN), the same view one row later is clean"""
    H, W, C = 6, 5, 8
    ar = A.Arena("cpu")
    g = torch.Generator().manual_seed(1)
    x = ar.put(torch.randint(-2, 3, (H, W, C), generator=g).double(), BF, name="x")
    op = ar.operand(x)
    row = W * C * 2
    early = op.buf[op.lo - row: op.lo - row + op.nbytes].view(BF).view(1, H, W, C).permute(0, 3, 1, 2).float()
    w = torch.zeros(4, C, 3, 3)
    assert bool(torch.isnan(F.conv2d(early, w, padding=1)[0, :, :2]).all())
    assert not bool(torch.isnan(F.conv2d(early, w, padding=1)[0, :, 2:]).any())
    assert not bool(torch.isnan(F.conv2d(x.view(1, H, W, C).permute(0, 3, 1, 2).float(), w, padding=1)).any())
    u8 = ar.put(torch.randint(0, 255, (H, W, 3), generator=g, dtype=torch.int64).to(torch.uint8), name="img")
    table = torch.arange(256.0).repeat(3, 1)
    table[:, 255] = float("nan")
    o8 = ar.operand(u8)
    stray = o8.buf[o8.lo - 1: o8.lo - 1 + o8.nbytes].view(H, W, 3).long()
    assert bool(torch.isnan(table[0][stray]).any()) and not bool(torch.isnan(table[0][u8.long()]).any())


# ------------------------------------------------------------------------------------------------ completeness guard
def _defined_in_sources():
    names = set()
    for f in SOURCES:
        txt = open(os.path.join(CSRC, f)).read()
        names |= set(re.findall(r"^(?:extern \"C\" )?(?:int|long long) (vqa_\w+)\(", txt, flags=re.M))
    return names


def _pointer_entries():
    """entries of the header that the six sources define, that launch (take a stream) and take at least one device pointer"""
    L = sub("_lib")
    decl = L.parse_header(open(os.path.join(REPO, "include", "vqa_hip.h")).read())
    defined = _defined_in_sources()
    out = []
    for name, (_, names, ctypes_, has_stream) in decl.items():
        if name in defined and has_stream and any(t is L.P for t in ctypes_[:-1]):          # (host-only queries: exempt by rule)
            out.append(name)
    return sorted(out)


def test_every_pointer_taking_entry_is_covered_or_exempt_with_a_reason():
    import test_gpu_arena_gemm_conv as G
    entries = _pointer_entries()
    assert len(entries) >= 36 and "vqa_igemm" in entries and "vqa_conv8p" in entries and "vqa_stem_dgrad_fused" in entries
    assert "vqa_igemm_mtiles" not in entries and "vqa_wgrad_plan" not in entries
    assert not (G.COVERED & set(G.EXEMPT)), sorted(G.COVERED & set(G.EXEMPT))
    missing = [e for e in entries if e not in G.COVERED and e not in G.EXEMPT]
    assert not missing, f"no arena case and no exemption for: {missing}"
    stale = [e for e in list(G.COVERED) + list(G.EXEMPT) if e not in entries]
    assert not stale, f"listed but not a pointer-taking entry of {SOURCES}: {stale}"
    for e, why in G.EXEMPT.items():
        assert isinstance(why, str) and len(why.split()) >= 4 and "\n" not in why, e
    src = open(G.__file__).read()
    for e in G.COVERED:
        assert src.count('"%s"' % e) >= 2, f"{e} is listed as covered but no test names it"
