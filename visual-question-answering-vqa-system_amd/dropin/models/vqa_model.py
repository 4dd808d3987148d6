"""`models.vqa_model` drop-in backed by the HIP engine (reference: models/vqa_model.py).

Same constructor kwargs (:132-152), `forward(images, token_ids, attention_mask=None, return_aux=False)` (:243-311),
`.predict` (:313-339), `.get_attention_maps` (:341-369), `.get_num_parameters` (:371-380), `.config` (:226-241),
`create_vqa_model` (:383-407), `load_vqa_model` (:410-432) and the same 225 state_dict entries.
Extension (inference only): many questions per image from one image encoding -- `forward(..., image_index=)`,
`encode_images(images) -> ImageContext` and `answer(context, token_ids, ...)`.
Extension (training): `forward_grouped(images, token_ids, attention_mask, image_index)` runs one CNN pass per image and trains
through it; `group_by_image(image_ids)` turns a batch's image ids into that form.
Extension (inference only): `predict_topk(...)` / `answer_topk(context, ...)` return the k best answers with their probabilities
(`TopK`) from one extra launch inside the captured graph, with an optional answer whitelist and softmax temperature.
Extension (inference only): `explain(...)` returns Grad-CAM and cross-attention maps over the image-feature grid (`Explanation`) from
an eval-mode taped forward and a backward that stops at the image features; `Explanation.render(...)` turns one into uint8 pictures.
There is no CPU path: calling forward with CPU tensors, or without the built extension, raises.
"""
from __future__ import annotations

import importlib
import math
import os
from typing import Any, Callable, Dict, List, NamedTuple, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.optim.optimizer as _optim_hooks

def _pkg():
    import sys
    here = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # .../visual-question-answering-vqa-system_amd
    root = os.path.dirname(here)
    if root not in sys.path:
        sys.path.insert(0, root)
    return importlib.import_module(os.path.basename(here))


ByteImages = _pkg().load_dropin_byte_images().ByteImages       # uint8 HWC images as they are (dropin/utils/byte_images.py)


_is_bytes = _pkg().kernels.is_byte_images                      # (recognised by its members: utils.byte_images has several import names)

def _op_images(model, images: torch.Tensor):
    """The image operand of a custom op as the engine takes it: ops carry tensors only, so a ByteImages travels as its uint8 data
    (a plain uint8 tensor was cast to float before it got here) and is wrapped again with the mean / std forward() left behind."""
    return ByteImages(images, *model._byte_norm) if images.dtype == torch.uint8 else images


def _image_hw(images: torch.Tensor):
    """(H, W) of an op's image operand: NCHW floats, or the uint8 HWC data of a ByteImages."""
    return (images.shape[1], images.shape[2]) if images.dtype == torch.uint8 else (images.shape[2], images.shape[3])


class _Node(nn.Module):
    """Anonymous container; the module tree only exists to give parameters their reference names."""


# ----------------------------------------------------------------------------------------------------------------------
# torch custom ops: the whole HIP forward and backward are registered in the `vqa_hip` namespace
#   torch.ops.vqa_hip.vqa_forward(images, token_ids, mask, params, handle, training, want_aux) -> logits
#   torch.ops.vqa_hip.vqa_backward(dlogits, handle, tape_id) -> flat gradient buffer (layout.py slots)
#   torch.ops.vqa_hip.vqa_backward_input(dlogits, handle, tape_id, H, W) -> (flat gradient buffer, image gradient [B][3][H][W])
# with a fake (shape-only) implementation and an autograd formula, so the node is visible to the dispatcher, autograd,
# and FakeTensor tracing.  `handle` indexes a registry of live models (ops cannot carry Python objects); forward and
# backward are explicit kernel sequences over the C ABI (engine.py).
# ----------------------------------------------------------------------------------------------------------------------
_MODELS: Dict[int, "VQAModel"] = {}
_NEXT_HANDLE = [1]


@torch.library.custom_op("vqa_hip::vqa_forward", mutates_args=(), device_types="cuda")
def _vqa_forward_op(images: torch.Tensor, token_ids: torch.Tensor, mask: Optional[torch.Tensor], flat_params: torch.Tensor,
                    handle: int, training: bool, want_aux: bool) -> torch.Tensor:
    # flat_params: the model's ONE flat fp32 parameter buffer as an autograd-tracked alias (_FlatParams below).  Handing the dispatcher
    # the 164 parameter views as a List[Tensor] cost ~0.6 ms of host time per call before the first kernel went out -- idle GPU time
    # for a caller that synchronises every step (training/train.py:211)
    model = _MODELS[handle]
    plan, model._pending_plan = model._pending_plan, None
    logits, aux, tape = model._engine.forward(_op_images(model, images), token_ids, mask, training, want_aux, need_tape=True, plan=plan)
    model._last_aux = aux              # aux tensors are detached by construction (side channel, not graph outputs)
    model._tape_seq += 1
    model._tapes[model._tape_seq] = tape
    while len(model._tapes) > model.max_live_tapes:      # a forward whose backward never ran must not pin its activations forever
        model._tapes.pop(next(iter(model._tapes)))
    return logits


@_vqa_forward_op.register_fake
def _(images, token_ids, mask, flat_params, handle, training, want_aux):
    return images.new_empty((images.shape[0], _MODELS[handle].num_answers), dtype=torch.float32)


@torch.library.custom_op("vqa_hip::vqa_backward", mutates_args=(), device_types="cuda")
def _vqa_backward_op(dlogits: torch.Tensor, handle: int, tape_id: int) -> torch.Tensor:
    """Returns the FLAT gradient buffer (same layout as the flat parameter buffer); the autograd formula slices it."""
    model = _MODELS[handle]
    tape = model._tapes.pop(tape_id, None)
    if tape is None:
        raise RuntimeError(f"vqa_backward: the activations of forward #{tape_id} are gone -- either backward ran twice through it "
                           f"(the reference needs retain_graph=True for that) or more than max_live_tapes = {model.max_live_tapes} "
                           "training forwards were issued before its backward (raise VQAModel.max_live_tapes)")
    G = torch.zeros_like(model._flat)
    model._engine.backward(tape, dlogits.contiguous(), G, on_segment=model._on_segment)
    return G


@_vqa_backward_op.register_fake
def _(dlogits, handle, tape_id):
    return torch.empty_like(_MODELS[handle]._flat)


@torch.library.custom_op("vqa_hip::vqa_backward_input", mutates_args=(), device_types="cuda")
def _vqa_backward_input_op(dlogits: torch.Tensor, handle: int, tape_id: int, H: int, W: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """vqa_backward plus the gradient with respect to the images (fp32 NCHW [B][3][H][W]): the backward of a forward whose images
    require grad.  The parameter gradients are computed either way (a frozen model's are dropped by autograd)."""
    model = _MODELS[handle]
    tape = model._tapes.pop(tape_id, None)
    if tape is None:
        raise RuntimeError(f"vqa_backward: the activations of forward #{tape_id} are gone -- either backward ran twice through it "
                           f"(the reference needs retain_graph=True for that) or more than max_live_tapes = {model.max_live_tapes} "
                           "training forwards were issued before its backward (raise VQAModel.max_live_tapes)")
    G = torch.zeros_like(model._flat)
    dimg = model._engine.backward(tape, dlogits.contiguous(), G, on_segment=model._on_segment, want_input_grad=True)
    return G, dimg


@_vqa_backward_input_op.register_fake
def _(dlogits, handle, tape_id, H, W):
    return torch.empty_like(_MODELS[handle]._flat), dlogits.new_empty((dlogits.shape[0], 3, H, W), dtype=torch.float32)


# many questions per image in training (VQAModel.forward_grouped):
#   torch.ops.vqa_hip.vqa_forward_grouped(images [U], token_ids [N], mask, image_index int32 [N], params, handle, training) -> logits [N]
#   torch.ops.vqa_hip.vqa_backward_grouped_input(dlogits, handle, tape_id, U, H, W) -> (flat gradient, image gradient [U][3][H][W])
# The backward without an image gradient is vqa_backward itself (the engine's tape carries the image index).
@torch.library.custom_op("vqa_hip::vqa_forward_grouped", mutates_args=(), device_types="cuda")
def _vqa_forward_grouped_op(images: torch.Tensor, token_ids: torch.Tensor, mask: Optional[torch.Tensor], image_index: torch.Tensor,
                            flat_params: torch.Tensor, handle: int, training: bool) -> torch.Tensor:
    model = _MODELS[handle]
    plan, model._pending_plan = model._pending_plan, None
    logits, _, tape = model._engine.forward(_op_images(model, images), token_ids, mask, training, False, need_tape=True, kv_index=image_index,
                                            plan=plan)
    model._tape_seq += 1
    model._tapes[model._tape_seq] = tape
    while len(model._tapes) > model.max_live_tapes:
        model._tapes.pop(next(iter(model._tapes)))
    return logits


@_vqa_forward_grouped_op.register_fake
def _(images, token_ids, mask, image_index, flat_params, handle, training):
    return images.new_empty((token_ids.shape[0], _MODELS[handle].num_answers), dtype=torch.float32)


@torch.library.custom_op("vqa_hip::vqa_backward_grouped_input", mutates_args=(), device_types="cuda")
def _vqa_backward_grouped_input_op(dlogits: torch.Tensor, handle: int, tape_id: int, U: int, H: int, W: int) -> Tuple[torch.Tensor, torch.Tensor]:
    model = _MODELS[handle]
    tape = model._tapes.pop(tape_id, None)
    if tape is None:
        raise RuntimeError(f"vqa_backward: the activations of forward #{tape_id} are gone -- either backward ran twice through it "
                           f"(the reference needs retain_graph=True for that) or more than max_live_tapes = {model.max_live_tapes} "
                           "training forwards were issued before its backward (raise VQAModel.max_live_tapes)")
    G = torch.zeros_like(model._flat)
    dimg = model._engine.backward(tape, dlogits.contiguous(), G, on_segment=model._on_segment, want_input_grad=True)
    return G, dimg


@_vqa_backward_grouped_input_op.register_fake
def _(dlogits, handle, tape_id, U, H, W):
    return torch.empty_like(_MODELS[handle]._flat), dlogits.new_empty((U, 3, H, W), dtype=torch.float32)


def _grouped_setup_ctx(ctx, inputs, output):
    handle = inputs[5]
    ctx.handle = handle
    ctx.tape_id = _MODELS[handle]._tape_seq
    ctx.image_shape = (inputs[0].shape[0],) + _image_hw(inputs[0])


def _grouped_backward(ctx, dlogits):
    if ctx.needs_input_grad[0]:
        G, dimg = torch.ops.vqa_hip.vqa_backward_grouped_input(dlogits, ctx.handle, ctx.tape_id, *ctx.image_shape)
        return dimg, None, None, None, G, None, None
    G = torch.ops.vqa_hip.vqa_backward(dlogits, ctx.handle, ctx.tape_id)
    return None, None, None, None, G, None, None


torch.library.register_autograd("vqa_hip::vqa_forward_grouped", _grouped_backward, setup_context=_grouped_setup_ctx)


# training from cached image features (ImageFeatures; the image encoder is frozen, in eval mode and never runs):
#   torch.ops.vqa_hip.vqa_forward_features(features [U][Hf][Wf][Cf], token_ids [N], mask, image_index int32 [N] | None, params, handle,
#                                          training) -> logits [N]
# The backward is vqa_backward itself: the tape's plan has no CNN part, and the features get no gradient.
@torch.library.custom_op("vqa_hip::vqa_forward_features", mutates_args=(), device_types="cuda")
def _vqa_forward_features_op(features: torch.Tensor, token_ids: torch.Tensor, mask: Optional[torch.Tensor],
                             image_index: Optional[torch.Tensor], flat_params: torch.Tensor, handle: int, training: bool) -> torch.Tensor:
    model = _MODELS[handle]
    plan, model._pending_plan = model._pending_plan, None
    logits, _, tape = model._engine.forward_features(features, token_ids, mask, training, False, need_tape=True, kv_index=image_index,
                                                     plan=plan)
    model._tape_seq += 1
    model._tapes[model._tape_seq] = tape
    while len(model._tapes) > model.max_live_tapes:
        model._tapes.pop(next(iter(model._tapes)))
    return logits


@_vqa_forward_features_op.register_fake
def _(features, token_ids, mask, image_index, flat_params, handle, training):
    return features.new_empty((token_ids.shape[0], _MODELS[handle].num_answers), dtype=torch.float32)


def _features_setup_ctx(ctx, inputs, output):
    ctx.handle = inputs[5]
    ctx.tape_id = _MODELS[inputs[5]]._tape_seq


def _features_backward(ctx, dlogits):
    G = torch.ops.vqa_hip.vqa_backward(dlogits, ctx.handle, ctx.tape_id)
    return None, None, None, None, G, None, None


torch.library.register_autograd("vqa_hip::vqa_forward_features", _features_backward, setup_context=_features_setup_ctx)


def _setup_ctx(ctx, inputs, output):
    handle = inputs[4]
    ctx.handle = handle
    ctx.tape_id = _MODELS[handle]._tape_seq
    ctx.image_hw = _image_hw(inputs[0])


def _backward(ctx, dlogits):
    if ctx.needs_input_grad[0]:           # the images require grad: the stem's data gradient runs too
        G, dimg = torch.ops.vqa_hip.vqa_backward_input(dlogits, ctx.handle, ctx.tape_id, *ctx.image_hw)
        return dimg, None, None, G, None, None, None
    G = torch.ops.vqa_hip.vqa_backward(dlogits, ctx.handle, ctx.tape_id)
    return None, None, None, G, None, None, None


torch.library.register_autograd("vqa_hip::vqa_forward", _backward, setup_context=_setup_ctx)


# ----------------------------------------------------------------------------------------------------------------------
# graph-connected aux outputs: forward(..., return_aux=True) under autograd is three chained ops, split where the engine's backward
# reports its segments (engine.backward_head / _fusion / _encoders):
#   vqa_aux_encoders(images, token_ids, mask, params, handle, training) -> image_features, text_features
#   vqa_aux_fusion(image_features, text_features, handle, tape_id)       -> fused, image_projected, cross_attention_weights (stacked),
#                                                                           attended_pooled, text_pooled
#   vqa_aux_head(fused, handle, tape_id)                                  -> logits
# The forward is still ONE engine pass (issued by the encoders op; the other two hand out what it computed), so values and launches
# are those of vqa_forward.  Each op's backward runs its part of the engine backward; the parameter gradients of all three parts
# accumulate into one flat buffer per forward and backward pass, which the encoders op (the last node of every backward that reaches
# the parameters) returns.  A pass that ends before the encoders node (autograd.grad w.r.t. an aux tensor) drops that buffer with
# it.  Gradients on the aux tensors enter where those tensors enter the backward; autograd itself sums the gradients of
# image_features / text_features / fused with those of their consumers.
# ----------------------------------------------------------------------------------------------------------------------
def _aux_tape(model, tape_id, part):
    tape = model._tapes.get(tape_id)
    if tape is None or part not in tape:
        raise RuntimeError(f"vqa_backward: the activations of forward #{tape_id} are gone -- either backward ran twice through it "
                           f"(the reference needs retain_graph=True for that) or more than max_live_tapes = {model.max_live_tapes} "
                           "training forwards were issued before its backward (raise VQAModel.max_live_tapes)")
    return tape


_AUX_SEGMENTS = ("answer_head", "fusion")     # segments of the head / fusion parts, reported in this order before the encoders' ones


def _aux_grad_buffer(model, tape):
    """The flat gradient buffer of the CURRENT backward pass through this forward (created by the first of its nodes that runs)."""
    if tape.get("_G") is None:
        tape["_G"] = torch.zeros_like(model._flat)
        tape["_reported"] = set()

        def end_of_pass():
            # a pass that reached the encoders node has handed the buffer out already; otherwise what the head / fusion nodes put
            # there belongs to a backward that did not ask for parameter gradients: dropped, never returned by a later pass
            tape.pop("_G", None)
            tape.pop("_reported", None)
        torch.autograd.Variable._execution_engine.queue_callback(end_of_pass)
    return tape["_G"]


def _report_skipped_segments(model, tape, upto):
    """Segments of the parts before `upto` that this pass did not run (a loss on aux alone skips the head; one on image_features
    alone skips the fusion part too): their parameters' gradients are the buffer's zeros, and a reducer driven by on_segment still
    sees every bucket, in the usual order."""
    for name in _AUX_SEGMENTS[:upto]:
        if name not in tape["_reported"]:
            tape["_reported"].add(name)
            if model._on_segment is not None:
                ev = torch.cuda.Event(); ev.record(torch.cuda.current_stream())
                model._on_segment(name, [ev])


def _to_f32(model, t):
    """Compute-dtype gradient -> fp32 (the dtype of the public aux tensors)."""
    if t.dtype == torch.float32:
        return t
    out = torch.empty(t.shape, device=t.device, dtype=torch.float32)
    model._pkg._lib.call("vqa_convert", 1, 0, t.data_ptr(), out.data_ptr(), t.numel())
    return out


def _from_f32(model, g):
    """fp32 gradient of a public aux tensor -> compute dtype (a copy only where the dtypes differ)."""
    g = g.contiguous()
    if model.compute_dtype == torch.float32:
        return g
    out = torch.empty(g.shape, device=g.device, dtype=model.compute_dtype)
    model._pkg._lib.call("vqa_convert", 0, 1, g.data_ptr(), out.data_ptr(), g.numel())
    return out


def _final_hw(h):
    h = (h + 6 - 7) // 2 + 1            # stem conv 7x7 / 2
    h = (h + 2 - 3) // 2 + 1            # max pool 3x3 / 2
    for _ in range(3):                  # stages 2-4 open with a stride-2 block
        h = (h + 2 - 3) // 2 + 1
    return h


@torch.library.custom_op("vqa_hip::vqa_aux_encoders", mutates_args=(), device_types="cuda")
def _aux_encoders_op(images: torch.Tensor, token_ids: torch.Tensor, mask: Optional[torch.Tensor], flat_params: torch.Tensor,
                     handle: int, training: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    model = _MODELS[handle]
    plan, model._pending_plan = model._pending_plan, None
    logits, aux, tape = model._engine.forward(_op_images(model, images), token_ids, mask, training, True, need_tape=True, plan=plan)
    hw = tuple(_final_hw(v) for v in _image_hw(images))
    if tuple(aux["image_features"].shape[1:]) != (512,) + hw:              # the fake below derives the same shape from the geometry
        raise RuntimeError(f"image_features {tuple(aux['image_features'].shape)} disagrees with the stem / stage geometry {hw}")
    tape["_aux"] = (logits, aux)
    model._tape_seq += 1
    model._tapes[model._tape_seq] = tape
    while len(model._tapes) > model.max_live_tapes:
        model._tapes.pop(next(iter(model._tapes)))
    return aux["image_features"], aux["text_features"]


@_aux_encoders_op.register_fake
def _(images, token_ids, mask, flat_params, handle, training):
    m = _MODELS[handle]
    B, L = token_ids.shape
    H, W = _image_hw(images)
    return (images.new_empty((images.shape[0], 512, _final_hw(H), _final_hw(W)), dtype=torch.float32),
            images.new_empty((B, L, m.embed_dim), dtype=torch.float32))


def _aux_encoders_setup(ctx, inputs, output):
    ctx.set_materialize_grads(False)
    ctx.handle = inputs[4]
    ctx.tape_id = _MODELS[inputs[4]]._tape_seq


def _aux_encoders_bwd(ctx, dfeat, dtext):
    model = _MODELS[ctx.handle]
    tape = _aux_tape(model, ctx.tape_id, "stages")
    G = _aux_grad_buffer(model, tape)
    _report_skipped_segments(model, tape, 2)
    eng = model._engine
    if dfeat is not None:
        B, C, H, W = dfeat.shape
        g, dfeat = dfeat.contiguous(), torch.empty((B * H * W, C), device=dfeat.device, dtype=model.compute_dtype)
        model._pkg._lib.call("vqa_nchw_to_nhwc", model._pkg._lib.dt(model.compute_dtype), g.data_ptr(), dfeat.data_ptr(), B, H * W, C)
    if dtext is not None:
        dtext = _from_f32(model, dtext).view(-1, dtext.shape[-1])
    dimg = eng.backward_encoders(tape, dfeat, dtext, G, on_segment=model._on_segment, want_input_grad=ctx.needs_input_grad[0])
    model._tapes.pop(ctx.tape_id, None)
    tape.pop("_G", None)
    return dimg, None, None, G, None, None


torch.library.register_autograd("vqa_hip::vqa_aux_encoders", _aux_encoders_bwd, setup_context=_aux_encoders_setup)


@torch.library.custom_op("vqa_hip::vqa_aux_fusion", mutates_args=(), device_types="cuda")
def _aux_fusion_op(image_features: torch.Tensor, text_features: torch.Tensor, handle: int,
                   tape_id: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    model = _MODELS[handle]
    tape = _aux_tape(model, tape_id, "pool")
    _, aux = tape["_aux"]
    att, txt = aux["attended_pooled"], aux["text_pooled"]
    if att.untyped_storage().data_ptr() == txt.untyped_storage().data_ptr():
        txt = txt.clone()                 # fp32: both are column halves of one buffer; the outputs of an op may not alias
    caw = tape.get("caw")
    if caw is None:                       # no cross-attention layer: an empty stack
        B, ntok, _ = aux["image_projected"].shape
        caw = att.new_empty((0, B, model.config["num_attention_heads"], aux["text_features"].shape[1], ntok))
    return aux["fused"], aux["image_projected"], caw, att, txt


@_aux_fusion_op.register_fake
def _(image_features, text_features, handle, tape_id):
    m = _MODELS[handle]
    B, L, d = text_features.shape
    ntok = image_features.shape[2] * image_features.shape[3]
    heads, ncl = m.config["num_attention_heads"], m.config["num_cross_layers"]
    e = image_features.new_empty
    return e((B, d)), e((B, ntok, d)), e((ncl, B, heads, L, ntok)), e((B, d)), e((B, d))


def _aux_fusion_setup(ctx, inputs, output):
    ctx.set_materialize_grads(False)
    ctx.handle, ctx.tape_id = inputs[2], inputs[3]
    ctx.text_shape = tuple(inputs[1].shape)
    ctx.feat_shape = tuple(inputs[0].shape)


def _aux_fusion_bwd(ctx, dfused, dimg, dcaw, datt, dtxt):
    model = _MODELS[ctx.handle]
    tape = _aux_tape(model, ctx.tape_id, "pool")
    G = _aux_grad_buffer(model, tape)
    _report_skipped_segments(model, tape, 1)
    taps = {"image_projected": dimg, "attended_pooled": datt, "text_pooled": dtxt,
            "cross_attention_weights": None if dcaw is None else dcaw.unbind(0)}
    dfeat, denc = model._engine.backward_fusion(tape, dfused, G, on_segment=model._on_segment, taps=taps)
    tape["_reported"].add("fusion")
    B, C, H, W = ctx.feat_shape
    dfeat_nchw = torch.empty(ctx.feat_shape, device=dfeat.device, dtype=torch.float32)
    model._pkg._lib.call("vqa_nhwc_to_nchw", model._pkg._lib.dt(dfeat), dfeat.data_ptr(), dfeat_nchw.data_ptr(), B, H * W, C)
    return dfeat_nchw, _to_f32(model, denc).view(ctx.text_shape), None, None


torch.library.register_autograd("vqa_hip::vqa_aux_fusion", _aux_fusion_bwd, setup_context=_aux_fusion_setup)


@torch.library.custom_op("vqa_hip::vqa_aux_head", mutates_args=(), device_types="cuda")
def _aux_head_op(fused: torch.Tensor, handle: int, tape_id: int) -> torch.Tensor:
    tape = _aux_tape(_MODELS[handle], tape_id, "head")
    logits, _ = tape.pop("_aux")
    return logits


@_aux_head_op.register_fake
def _(fused, handle, tape_id):
    return fused.new_empty((fused.shape[0], _MODELS[handle].num_answers), dtype=torch.float32)


def _aux_head_setup(ctx, inputs, output):
    ctx.handle, ctx.tape_id = inputs[1], inputs[2]


def _aux_head_bwd(ctx, dlogits):
    model = _MODELS[ctx.handle]
    tape = _aux_tape(model, ctx.tape_id, "head")
    G = _aux_grad_buffer(model, tape)
    dfused = model._engine.backward_head(tape, dlogits, G, on_segment=model._on_segment)
    tape["_reported"].add("answer_head")
    return _to_f32(model, dfused), None, None


torch.library.register_autograd("vqa_hip::vqa_aux_head", _aux_head_bwd, setup_context=_aux_head_setup)


class _FlatParams(torch.autograd.Function):
    """The flat parameter buffer as a function of the 164 leaf Parameters that are views into it: forward aliases the buffer (no
    copy), backward hands each Parameter its slice of the flat gradient (views of ONE tensor, as `.grad` wants them for the flat
    optimizer paths).  A plain autograd.Function with 164 inputs costs ~0.15 ms of host time; the custom op behind it takes one tensor."""

    @staticmethod
    def forward(ctx, flat, handle, *params):
        ctx.handle = handle
        return flat.detach()

    @staticmethod
    def backward(ctx, G):
        model = _MODELS[ctx.handle]
        lay = model._pkg.layout
        return (None, None) + tuple(lay.view_of(G, e) for e in model._param_entries)


# torch.optim steps counted process-wide: an optimizer may write the parameters without bumping their version counters (its foreach
# kernels work on aliases), so any step makes every ImageContext stale (a server that trains nothing in-process never pays for it)
_OPT_STEPS = [0]
_OPT_PRE: Dict[int, Dict[int, int]] = {}      # id(optimizer) -> {model handle: _feat_version()} while that optimizer's step() runs


def _before_optimizer_step(optimizer, args, kwargs):
    # only models that ever handed out an ImageFeatures are looked at: a process that caches no features pays one dict scan per step.
    # (A step that raises leaves its entry behind until that optimizer's next step overwrites it: one small dict per optimizer.)
    pre = {h: m._feat_version() for h, m in _MODELS.items() if m._feat_live}
    if pre:
        _OPT_PRE[id(optimizer)] = pre
    else:
        _OPT_PRE.pop(id(optimizer), None)


def _count_optimizer_step(optimizer, args, kwargs):
    _OPT_STEPS[0] += 1
    # cached image features (VQAModel._feat_stamp): a step that wrote an image_encoder parameter (the optimizer writes exactly the
    # parameters that hold a gradient) makes them stale; what any other step did to the version counters _feat_version reads is excused
    before = _OPT_PRE.pop(id(optimizer), None)
    live = [(h, m) for h, m in _MODELS.items() if m._feat_live]
    if not live:
        return
    written = {id(p) for g in optimizer.param_groups for p in g["params"] if p.grad is not None}
    for h, m in live:
        if before is None or h not in before or any(id(p) in written for p in m._cnn_params()):
            m._feat_epoch += 1                  # (no reading from before the step -- the features were made inside it: nothing to excuse by)
        else:
            m._feat_excused += m._feat_version() - before[h]


_optim_hooks.register_optimizer_step_pre_hook(_before_optimizer_step)
_optim_hooks.register_optimizer_step_post_hook(_count_optimizer_step)


class TopK(NamedTuple):
    """The k best answers of N questions (VQAModel.predict_topk / answer_topk): best first, ties by the lower index."""
    indices: torch.Tensor                    # int64 [N, k]
    probs: torch.Tensor                      # float32 [N, k]
    logits: Optional[torch.Tensor] = None    # float32 [N, num_answers] when return_logits=True

    def to_records(self, decode: Callable[[int], str]) -> List[Dict]:
        """Per question the dictionary of api/inference.py:236-253 without its 'question' key; decode maps an answer index to its
        string (the answer vocabulary's decode).  Two read-backs for the whole batch (one .tolist() per tensor)."""
        out = []
        for irow, prow in zip(self.indices.tolist(), self.probs.tolist()):
            answers = [{"answer": decode(i), "probability": p, "index": i} for i, p in zip(irow, prow)]
            out.append({"answers": answers, "top_answer": answers[0]["answer"], "confidence": answers[0]["probability"]})
        return out


EXPLAIN_METHODS = ("gradcam", "attention")


class Explanation(NamedTuple):
    """Where the model looked for N questions (VQAModel.explain): maps over the image-feature grid, on the device."""
    logits: torch.Tensor                     # float32 [N, num_answers]: the eval-mode taped forward's
    answers: torch.Tensor                    # int64 [N]: the class each map explains (given, or the arg-max of logits)
    gradcam: Optional[torch.Tensor] = None   # float32 [N, Hf, Wf]: Grad-CAM of the image features for that class
    attention: Optional[torch.Tensor] = None   # float32 [N, Hf, Wf]: cross-attention, mean over layers, heads and real tokens

    def render(self, which: str = "gradcam", base=None, alpha: float = 0.5, colormap: Optional[torch.Tensor] = None,
               size: Optional[Tuple[int, int]] = None) -> torch.Tensor:
        """The map `which` as pictures, uint8 [N, H, W, 3] on the device, one launch (kernels.heatmap_render): upsampled bilinearly
        (F.interpolate, align_corners=False), looked up in `colormap` (uint8 [256, 3]; None: kernels.default_colormap()) and blended
        over `base` as alpha * colour + (1 - alpha) * base.  base: a ByteImages, a uint8 [N, H, W, 3] device tensor, or None (the
        colours alone).  size = (H, W) defaults to the base's and is required without one.  Map values are taken as [0, 1] (what
        explain(normalize=True) returns; others are clamped, a NaN takes the table's first entry).  ValueError for a map that was not
        computed, an alpha outside [0, 1], or a base / colour table / size of the wrong type or shape."""
        K = _pkg().kernels
        alpha = K.check_alpha(alpha)
        if which not in EXPLAIN_METHODS:
            raise ValueError(f"render: `which` must be one of {EXPLAIN_METHODS}, got {which!r}")
        maps = getattr(self, which)
        if maps is None:
            raise ValueError(f"render: this Explanation holds no {which!r} map (ask explain() for it with methods=)")
        if _is_bytes(base):
            base = base.data
        return K.heatmap_render(maps, size=size, base=base, alpha=alpha, colormap=colormap)


class ImageContext:
    """The image half of the eval forward for U images (VQAModel.encode_images): every cross-attention layer's K | V per image token,
    plus the NHWC features and projected tokens when made for aux.  Opaque; valid while the model's parameters, BatchNorm buffers
    (through load_state_dict) and inference precision stay as they were when it was made -- answer() refuses it afterwards."""
    __slots__ = ("num_images", "_eng", "_stamp", "_handle")

    def __init__(self, num_images: int, eng_ctx: dict, stamp: tuple, handle: int):
        self.num_images = num_images
        self._eng = eng_ctx
        self._stamp = stamp
        self._handle = handle

    def __repr__(self):
        return f"ImageContext(num_images={self.num_images})"


def _checked_index(index, U: int, what: str) -> torch.Tensor:
    """A 1-D integer index with every entry in [0, U), as given (any integer dtype, CPU or device): ValueError for another shape or
    dtype, IndexError for an entry out of range.  The range check is free for a CPU index and one device-to-host read for a device
    index (VQAModel._image_index's rule)."""
    if not isinstance(index, torch.Tensor):
        index = torch.as_tensor(index)
    if index.dim() != 1:
        raise ValueError(f"{what} must be 1-D; got shape {tuple(index.shape)}")
    if index.dtype.is_floating_point or index.dtype.is_complex or index.dtype == torch.bool:
        raise ValueError(f"{what} must hold integers, got {index.dtype}")
    if index.shape[0]:
        lo, hi = (int(v) for v in torch.stack(torch.aminmax(index)).tolist())
        if lo < 0 or hi >= U:
            raise IndexError(f"{what} holds {lo if lo < 0 else hi}, outside [0, {U}) for {U} images")
    return index


class ImageFeatures:
    """The image encoder's output for U images (VQAModel.encode_features): NHWC features [U, Hf, Wf, Cf] in the compute dtype on the
    device -- 50 KB per image at the default shape in bf16, so a dataset-sized bank stays resident.  Everything that takes images for a
    frozen, eval-mode image encoder takes one of these instead and skips the CNN: model(...), forward_grouped, encode_images,
    HipTrainer.step.  Valid while the image encoder's parameters and BatchNorm buffers are what they were when it was made (writes to
    the text encoder, fusion and answer head do not matter); refused with RuntimeError afterwards (VQAModel._feat_stamp)."""
    __slots__ = ("_t", "_stamp", "_handle")

    def __init__(self, t: torch.Tensor, stamp: tuple, handle: int):
        self._t = t
        self._stamp = stamp
        self._handle = handle

    @property
    def num_images(self) -> int:
        return self._t.shape[0]

    def tensor(self) -> torch.Tensor:
        """The device tensor [U, Hf, Wf, Cf] itself (not a copy): for torch.save; VQAModel.features_from_tensor wraps it again."""
        return self._t

    def select(self, index) -> "ImageFeatures":
        """The features of the images index[i], in that order (repeats allowed), as a new [len(index), Hf, Wf, Cf] block: one
        vqa_gather_rows launch.  index: 1-D, any integer dtype, CPU or device; the range check is free for a CPU index (which then
        goes to the device without a sync) and costs one device-to-host read for a device index.  ValueError for a wrong shape or
        dtype, IndexError for an entry outside [0, num_images), both before any launch."""
        model = _MODELS[self._handle]
        index = _checked_index(index, self.num_images, "ImageFeatures.select: index")
        dev = self._t.device
        if index.device != dev:
            index = index.to(torch.int32).pin_memory().to(dev, non_blocking=True) if dev.type == "cuda" else index.to(dev, torch.int32)
        else:
            index = index.to(torch.int32)
        return ImageFeatures(model._pkg.kernels.gather_rows(self._t, index.contiguous()), self._stamp, self._handle)

    @staticmethod
    def cat(parts) -> "ImageFeatures":
        """The features of several encode_features() calls as one block, in order.  All parts must come from one model in one state."""
        parts = list(parts)
        if not parts or any(not isinstance(p, ImageFeatures) for p in parts):
            raise ValueError("ImageFeatures.cat needs a non-empty sequence of ImageFeatures")
        if any(p._handle != parts[0]._handle or p._stamp != parts[0]._stamp for p in parts):
            raise RuntimeError("ImageFeatures.cat: the parts were made by different models, or the image encoder changed between them")
        return ImageFeatures(torch.cat([p._t for p in parts], dim=0), parts[0]._stamp, parts[0]._handle)

    def __repr__(self):
        return f"ImageFeatures(num_images={self.num_images}, shape={tuple(self._t.shape[1:])}, dtype={self._t.dtype})"


class VQAModel(nn.Module):
    def __init__(self, vocab_size: int = 10000, embed_dim: int = 256, num_answers: int = 1000,
                 use_se_attention: bool = True, use_spatial_attention: bool = True, se_reduction: int = 16,
                 num_transformer_layers: int = 4, num_attention_heads: int = 8, ffn_hidden_dim: int = 1024,
                 max_question_length: int = 20, num_cross_layers: int = 2, use_gating: bool = True,
                 dropout: float = 0.1, answer_dropout: float = 0.3, compute_dtype: Optional[str] = None, seed: Optional[int] = None,
                 num_image_tokens: int = 49):
        # compute_dtype / seed / num_image_tokens are extensions; the reference hard-codes 49 image positions (models/fusion.py:66),
        # num_image_tokens = 144 is the 384x384 stress shape of BASELINE configs[4]
        super().__init__()
        assert embed_dim % num_attention_heads == 0, \
            f"embed_dim ({embed_dim}) must be divisible by num_heads ({num_attention_heads})"
        self._pkg = _pkg()
        lay = self._pkg.layout
        self.embed_dim, self.num_answers = embed_dim, num_answers
        self.config = dict(vocab_size=vocab_size, embed_dim=embed_dim, num_answers=num_answers,
                           use_se_attention=use_se_attention, use_spatial_attention=use_spatial_attention,
                           se_reduction=se_reduction, num_transformer_layers=num_transformer_layers,
                           num_attention_heads=num_attention_heads, ffn_hidden_dim=ffn_hidden_dim,
                           max_question_length=max_question_length, num_cross_layers=num_cross_layers,
                           use_gating=use_gating, dropout=dropout, answer_dropout=answer_dropout)
        if num_image_tokens != 49:
            self.config["num_image_tokens"] = int(num_image_tokens)
        cd = (compute_dtype or os.environ.get("VQA_HIP_DTYPE", "bf16")).lower()
        self.compute_dtype = {"bf16": torch.bfloat16, "bfloat16": torch.bfloat16, "fp32": torch.float32, "float32": torch.float32}[cd]
        self._entries = lay.build_entries(self.config)
        self._param_entries = [e for e in self._entries if e.is_param]
        self._flat = torch.zeros(lay.flat_size(self._entries), dtype=torch.float32)
        gen = torch.Generator()
        gen.manual_seed(torch.initial_seed() if seed is None else seed)
        fan: Dict[str, int] = {}
        for e in self._entries:
            val = lay.init_value(e, self.config, gen, fan)
            node = self
            *path, leaf = e.name.split(".")
            for part in path:
                if not hasattr(node, part):
                    node.add_module(part, _Node())
                node = getattr(node, part)
            if e.is_param:
                view = lay.view_of(self._flat, e)
                view.copy_(val)
                node.register_parameter(leaf, nn.Parameter(view))
            else:
                node.register_buffer(leaf, val)
        self.image_encoder.output_channels = 512
        self.image_encoder.output_spatial_size = int(round(num_image_tokens ** 0.5))   # 7 in the reference (models/cnn_backbone.py:415)
        self.fusion.get_attention_visualization = self._attention_visualization
        self._engine = None
        self._infer_precision = "bf16"             # residual-block convs of the eval (Conv+BN folded) path: set_inference_precision
        self._on_segment = None
        self._pending_plan = None                   # fine-tuning plan handed to the next custom-op forward (finetune.Plan)
        self._byte_norm = None                      # (mean, std) of the ByteImages whose uint8 data the next custom-op forward carries
        self._plan_cache: Dict[str, Any] = {}
        self._last_aux = None
        self._tapes: Dict[int, Any] = {}
        self._graphs: Dict[Any, Any] = {}           # captured inference graphs, one per input shape (forward_graphed)
        self._tape_seq = 0
        self._ctx_epoch = 0                         # bumped by whatever invalidates an ImageContext torch cannot see (_ctx_stamp)
        self._feat_epoch = 0                        # bumped by whatever changes the image encoder (_feat_stamp)
        self._feat_excused = 0                      # flat-buffer version bumps known to have left the image encoder alone (_feat_stamp)
        self._feat_live = False                     # an ImageFeatures was handed out: the optimizer step hooks look at this model
        self._handle = _NEXT_HANDLE[0]
        _NEXT_HANDLE[0] += 1
        _MODELS[self._handle] = self

    def _param_list(self):
        # the 164 Parameter objects never change identity (.to() only swaps their .data), but resolving 164 dotted names through
        # nn.Module.__getattr__ on every forward cost the unchanged train.py loop a few hundred host microseconds with the GPU idle
        pl = self.__dict__.get("_params_cache")
        if pl is not None:
            # nn.Module._apply may REPLACE Parameter objects (torch.__future__.set_overwrite_module_params_on_conversion) and a user
            # may re-register one: a stale list would route gradients to orphans (optimizer sees grad = None).  _reflatten drops the
            # cache; this two-lookup probe (first and last parameter) catches the re-registration case
            e0, e1 = self._param_entries[0], self._param_entries[-1]
            if getattr_path(self, e0.name) is not pl[0] or getattr_path(self, e1.name) is not pl[-1]:
                pl = None
        if pl is None:
            pl = [getattr_path(self, e.name) for e in self._param_entries]
            self.__dict__["_params_cache"] = pl
        return pl

    def _part_modes(self):
        """(image_encoder, text_encoder, fusion, answer_head) modes; NotImplementedError for a submodule whose mode differs from its
        part's.  The module lists are cached: one attribute read per module on each call."""
        mods = self.__dict__.get("_part_mods")
        if mods is None:
            mods = [(name, [(n, m) for n, m in getattr(self, name).named_modules(prefix=name)]) for name in self._pkg.finetune.PARTS]
            self.__dict__["_part_mods"] = mods
        out = []
        for name, ms in mods:
            mode = ms[0][1].training
            for _, m in ms:
                if m.training != mode:
                    return self._pkg.finetune.part_modes(self)       # (raises, naming the module)
            out.append(mode)
        return tuple(out)

    def _finetune_plan(self, params, images_grad: bool, training: bool):
        """Fine-tuning plan of this forward (finetune.Plan), or None for the plain route: every parameter trains and every part runs
        in mode `training`."""
        modes = self._part_modes()
        if modes != (training,) * 4 and len(set(modes)) == 1:
            modes = (training,) * 4                  # (HipTrainer: the caller's mode when the parts agree)
        return self._pkg.finetune.resolve(self._param_entries, params, modes, images_grad, self._plan_cache)

    def _modes_plan(self, modes=None, taped=False):
        """A plan that only sets the part modes (everything computed): for forwards without a tape, and the aux graph ops.  None when
        the parts agree."""
        modes = self._part_modes() if modes is None else modes
        if len(set(modes)) == 1:
            return None
        return self._pkg.finetune.Plan(self._param_entries, (True,) * len(self._param_entries), modes, taped)

    def __del__(self):
        _MODELS.pop(getattr(self, "_handle", -1), None)

    # ---- storage management: parameters are views into one flat buffer; keep that true across .to()/.cuda()
    def _reflatten(self):
        lay = self._pkg.layout
        named = dict(self.named_parameters())
        dev = named[self._param_entries[0].name].device
        flat = torch.zeros(self._flat.numel(), dtype=torch.float32, device=dev)
        for e in self._param_entries:
            p = named[e.name]
            v = lay.view_of(flat, e)
            v.copy_(p.data.to(torch.float32))
            p.data = v
            if p.grad is not None:
                p.grad = None
        self._flat = flat
        self._engine = None
        self._ctx_epoch += 1
        self._feat_epoch += 1
        self.__dict__.pop("_params_cache", None)
        if self._graphs:                             # captured graphs hold the OLD flat buffer's pointers
            torch.cuda.synchronize()
            self._graphs.clear()

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self._reflatten()
        return out

    def _ensure_engine(self):
        if self._engine is None:
            if not self._flat.is_cuda:
                raise RuntimeError("VQAModel (HIP) needs its parameters on the GPU: call model.to('cuda'); there is no CPU path")
            bufs = {n: b for n, b in self.named_buffers()}
            self._engine = self._pkg.engine.HipEngine(self.config, self._entries, self._flat, bufs, self.compute_dtype)
        self._engine.infer_precision = self._infer_precision      # the setting lives here: .to() / _reflatten recreate the engine
        return self._engine

    # ---- inference precision (extension)
    INFERENCE_PRECISIONS = ("bf16", "mxfp8")

    @property
    def inference_precision(self) -> str:
        return self._infer_precision

    def set_inference_precision(self, precision: str) -> "VQAModel":
        """Precision of the residual-block convolutions where the Conv+BN-folded eval path runs (eval mode without autograd: eager
        eval forward, forward_graphed, predict, and return_aux / get_attention_maps under no_grad).  "bf16" (default) or "mxfp8"
        (OCP MX: e4m3 elements, one E8M0 scale per 32 channels; activation scales computed per forward, weights quantized from the
        fold on every forward).  Training, forwards under autograd, parameters, buffers and state_dict are unaffected."""
        if precision not in self.INFERENCE_PRECISIONS:
            raise ValueError(f"inference precision must be one of {self.INFERENCE_PRECISIONS}, got {precision!r}")
        if precision == "mxfp8" and self.compute_dtype != torch.bfloat16:
            raise ValueError("inference precision 'mxfp8' needs compute_dtype='bf16' (this model computes in fp32)")
        self._infer_precision = precision
        self._ctx_epoch += 1
        self._feat_epoch += 1
        if self._engine is not None:
            self._engine.infer_precision = precision
        return self

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        try:
            return super().load_state_dict(state_dict, strict=strict, assign=assign)
        finally:
            self._ctx_epoch += 1                     # BatchNorm buffers are not views of the flat buffer: its version misses them
            self._feat_epoch += 1

    # ---- reference API
    def forward(self, images: torch.Tensor, token_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                return_aux: bool = False, image_index: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[Dict]]:
        """image_index (extension, inference only): images is [U, 3, H, W], token_ids [N, L] and question i is asked of image
        image_index[i]; the result equals forward(images[image_index], token_ids, attention_mask) while the image half runs once per
        image (see answer()).
        images may be a ByteImages (extension; utils/byte_images.py): the uint8 HWC batch as decoded, normalised inside the stem
        kernels -- every result equals forward(images.to_float(), ...) bit for bit; so may the images of forward_grouped,
        encode_images, encode_features, predict and predict_topk.  An image gradient needs float images (TypeError).
        images may be an ImageFeatures (extension; encode_features): the image encoder, frozen and in eval mode, does not run, and
        everything after it is this forward -- eval, or training under autograd with gradients to the other three parts (then
        image_index is forward_grouped's, and return_aux raises NotImplementedError)."""
        if isinstance(images, ImageFeatures):
            return self._forward_features(images, token_ids, attention_mask, return_aux, image_index)
        if not images.is_cuda:
            raise RuntimeError("VQAModel (HIP) got CPU inputs; this implementation only runs on an MI355X (no CPU fallback)")
        if image_index is not None:
            return self._forward_indexed(images, token_ids, attention_mask, return_aux, image_index)
        eng = self._ensure_engine()
        images, norm = self._image_operand(images)
        token_ids = token_ids.contiguous().long()
        maskf = None if attention_mask is None else attention_mask.contiguous().float()
        params = self._param_list()
        if torch.is_grad_enabled() and (images.requires_grad or any(p.requires_grad for p in params)):
            self._byte_norm = norm               # (the ops below carry tensors: _op_images wraps the bytes again)
            # tapes are kept by id (gradient accumulation / loss1 + loss2: several forwards, then their backwards), oldest dropped
            # beyond max_live_tapes.  Images that require grad take this path even when no parameter does (a frozen model under
            # saliency / adversarial attacks): the flat buffer then goes in untracked, so no parameter receives a .grad, and the
            # forward is the taped one (never the captured graph nor the folded eval path; BatchNorm uses its running statistics)
            if any(p.requires_grad for p in params):
                flat = _FlatParams.apply(self._flat, self._handle, *params)
            else:
                flat = self._flat
            # fine-tuning (frozen parameters, parts in different modes): the engine prunes what nothing needs (finetune.Plan)
            plan = self._finetune_plan(params, images.requires_grad, self.training)
            if return_aux:                   # aux tensors on the autograd graph (three chained ops, see vqa_aux_encoders above)
                self._pending_plan = None if plan is None else self._modes_plan(plan.modes, True)     # part modes only: nothing pruned
                return self._forward_aux_graph(images, token_ids, maskf, flat)
            self._pending_plan = plan
            logits = torch.ops.vqa_hip.vqa_forward(images, token_ids, maskf, flat, self._handle, self.training, return_aux)
            aux, self._last_aux = self._last_aux, None
        elif (self.graph_inference and not self.training and not return_aux and 0 < images.shape[0] <= self.graph_max_batch
              and not torch.cuda.is_current_stream_capturing()):
            # the serving case: api/inference.py:228,296 calls model(image, ids, mask) under no_grad at B = 1 ... a few; ~190 launches
            # of a few microseconds are host-bound there, so the captured HIP graph of this shape is replayed (same kernels, same
            # logits); the result is copied out of the graph's static buffer so callers own what they get, like the reference
            logits, aux = self.forward_graphed(self._eng_images(images, norm), token_ids, attention_mask).clone(), None
        else:
            logits, aux, _ = eng.forward(self._eng_images(images, norm), token_ids, maskf, self.training, return_aux, need_tape=False,
                                         plan=self._modes_plan())
        return (logits, aux) if return_aux else (logits, None)

    def _image_operand(self, images):
        """What every entry does with its `images` argument: (tensor, norm).  A float (or any plain) tensor becomes the contiguous
        float32 NCHW batch the kernels read and norm is None -- a plain uint8 tensor too: 0 ... 255 as floats, as ever.  A ByteImages
        gives its uint8 HWC data as it is and norm = (mean, std); its lookup table is made here, ahead of any graph capture."""
        if _is_bytes(images):
            self._pkg.kernels.u8_norm_table(images.data.device, images.mean, images.std)
            return images.data, (images.mean, images.std)
        return images.contiguous().float(), None

    @staticmethod
    def _eng_images(images: torch.Tensor, norm):
        """The engine's image operand from _image_operand's pair (also from a graph's static copy of the tensor)."""
        return images if norm is None else ByteImages(images, *norm)

    def _forward_aux_graph(self, images, token_ids, maskf, flat):
        feat, text = torch.ops.vqa_hip.vqa_aux_encoders(images, token_ids, maskf, flat, self._handle, self.training)
        tape_id = self._tape_seq
        fused, img, caw, att, txt = torch.ops.vqa_hip.vqa_aux_fusion(feat, text, self._handle, tape_id)
        logits = torch.ops.vqa_hip.vqa_aux_head(fused, self._handle, tape_id)
        aux = {"image_features": feat, "text_features": text, "text_pooled": txt, "fused": fused,
               "cross_attention_weights": list(caw.unbind(0)), "image_projected": img, "attended_pooled": att}
        return logits, aux

    def _forward_eager_eval(self, images, token_ids, maskf):
        logits, _, _ = self._ensure_engine().forward(images, token_ids, maskf, False, False, need_tape=False)
        return logits

    def forward_graphed(self, images: torch.Tensor, token_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Latency mode for serving (api/inference.py:228,296 calls model(...) in eval mode under no_grad at B = 1 ... 64, where
        ~190 launches of a few microseconds each are host-bound): the eval forward (Conv+BN folded) is captured once per input
        shape into a HIP graph and replayed; inputs are copied into the graph's static buffers.  Inference only: eval mode, no
        autograd, logits only.  Returns the graph's STATIC output buffer (valid until the next call with this shape; forward()
        hands out a copy).  The shape cache is LRU; a graph is only dropped after the stream that replayed it has drained."""
        if self.training:
            raise RuntimeError("forward_graphed is the inference path: call model.eval() first")
        if not images.is_cuda:
            raise RuntimeError("VQAModel (HIP) got CPU inputs; this implementation only runs on an MI355X (no CPU fallback)")
        images, norm = self._image_operand(images)           # (ByteImages: the static image buffer is uint8, and mean / std are in the key)
        key = (tuple(images.shape), tuple(token_ids.shape), attention_mask is not None, self._flat.data_ptr(), self._ensure_engine().fold_eval,
               getattr(self._engine, "fuse_stem_eval", None), self._infer_precision) + (() if norm is None else (norm,))
        g = self._graphs.pop(key, None)
        if g is None:
            st_img = images.detach().clone()
            st_ids = token_ids.detach().clone().contiguous().long()
            st_msk = None if attention_mask is None else attention_mask.detach().clone().contiguous().float()
            with torch.no_grad():
                graph, out = self._capture(lambda: self._forward_eager_eval(self._eng_images(st_img, norm), st_ids, st_msk))
            g = (graph, st_img, st_ids, st_msk, out)
        self._graph_put(key, g)                      # (re)inserted at the young end of the LRU order
        graph, st_img, st_ids, st_msk, out = g
        st_img.copy_(images); st_ids.copy_(token_ids)
        if st_msk is not None:
            st_msk.copy_(attention_mask)
        graph.replay()
        return out

    # ---- many questions per image (extension, inference only)
    def _ctx_stamp(self, eng):
        # what an ImageContext must still match: the flat buffer's version counter (load_state_dict, in-place writes through the
        # parameters), the process-wide torch.optim step count, the engine's training-forward count (train-mode forwards move BatchNorm
        # running statistics, and HipTrainer's AdamW writes the parameters through a raw pointer) and the model epoch
        # (load_state_dict, .to(), set_inference_precision).  Four integers: answer() at N = 1 is a latency path
        return (self._ctx_epoch, self._flat._version, _OPT_STEPS[0], eng.step_id)

    # ---- cached image features (extension)
    def _feat_stamp(self, eng):
        # What an ImageFeatures must still match.  Unlike an ImageContext it depends on the image encoder ALONE, and every AdamW step
        # of a fine-tuning run writes the other three parts, so _ctx_stamp's terms (whole-buffer version, every optimizer step, every
        # training forward) would refuse a bank after its first step.  Three host integers, nothing read from the device:
        #   _feat_epoch              bumped by load_state_dict, .to() (_reflatten), set_inference_precision, a HipTrainer step whose plan
        #                            trains an image_encoder parameter (trainer.py), a torch.optim step that wrote one (the step hooks
        #                            above: the optimizer writes the parameters that hold a gradient), ema_weights() unless the trainer
        #                            knows the average's image encoder equals the model's, and invalidate_features();
        #   eng.cnn_train_forwards   forwards that ran the CNN in train mode: BatchNorm running statistics moved;
        #   _feat_version - excused  torch's version counters of the flat buffer and of the image_encoder parameters: an in-place torch
        #                            write to one of those parameters (or to the flat buffer they are views of) moves them.  After
        #                            .to() every Parameter has a counter of its own, so writes to the other parts are not seen at all;
        #                            a model whose parameters still share the flat buffer's counter sees every write.  Bumps by writers
        #                            known to leave the image encoder alone are excused (_feat_excused: torch.optim steps that wrote no
        #                            image_encoder parameter, the ema_weights() exchange while the average still has this image encoder); any
        #                            other bump makes the features stale.  HipTrainer's AdamW writes through a raw pointer and moves
        #                            no counter.
        # Not seen (as HipTrainer.params_changed documents for the operand copy): writes through `.data` or a raw pointer, which
        # bypass torch's version counters; after one, call invalidate_features().
        self._feat_live = True
        return (self._feat_epoch, eng.cnn_train_forwards, self._feat_version() - self._feat_excused)

    def _feat_version(self):
        return self._flat._version + sum(p._version for p in self._cnn_params())

    def _cnn_params(self):
        pl = self._param_list()
        idx = self.__dict__.get("_cnn_param_idx")
        if idx is None:
            idx = [j for j, e in enumerate(self._param_entries) if e.name.startswith("image_encoder.")]
            self.__dict__["_cnn_param_idx"] = idx
        return [pl[j] for j in idx]

    def invalidate_features(self):
        """Declare every ImageFeatures made so far stale: for writes to the image encoder that torch's version counters do not see
        (through `.data`, a raw pointer or another C-ABI call)."""
        self._feat_epoch += 1

    def _check_features(self, features: "ImageFeatures", what: str):
        """The engine, after checking that `features` may stand in for this model's frozen, eval-mode image encoder: RuntimeError for
        another model's features, stale ones, a trainable image_encoder parameter while autograd records, or a train-mode image encoder
        -- all host logic, before any launch."""
        if features._handle != self._handle:
            raise RuntimeError(f"{what}: these ImageFeatures were made by another model")
        eng = self._ensure_engine()
        if features._stamp != self._feat_stamp(eng):
            raise RuntimeError(f"{what}: stale ImageFeatures: the image encoder's parameters, BatchNorm buffers or inference precision "
                               "changed since encode_features() made them; encode the images again")
        if self._part_modes()[0]:
            raise RuntimeError(f"{what}: ImageFeatures stand in for an eval-mode image encoder: call model.image_encoder.eval()")
        t = features._t
        if t.dim() != 4 or t.dtype != self.compute_dtype or t.device != self._flat.device or not t.is_contiguous():
            raise RuntimeError(f"{what}: the features must be a contiguous [U, Hf, Wf, Cf] {self.compute_dtype} tensor on {self._flat.device}")
        return eng

    def encode_features(self, images: torch.Tensor, out: Optional["ImageFeatures"] = None, at: int = 0) -> "ImageFeatures":
        """Run the image encoder alone, once per image, and keep its output: exactly the launches forward() issues for a frozen,
        eval-mode image encoder (stem and residual stages on the Conv+BN-folded path, set_inference_precision honoured), nothing after
        them.  Inference only, under encode_images' rules (eval mode, no autograd).  out / at: write the U results into rows
        [at, at + U) of an existing ImageFeatures (features_from_tensor(torch.empty(...)) makes an empty bank) and return it, so a
        dataset-sized bank is filled batch by batch; ImageFeatures.cat joins separate results instead."""
        if not images.is_cuda:
            raise RuntimeError("VQAModel (HIP) got CPU inputs; this implementation only runs on an MI355X (no CPU fallback)")
        self._inference_only("encode_features", images)
        eng = self._ensure_engine()
        if out is not None:
            if not isinstance(out, ImageFeatures):
                raise TypeError("encode_features: `out` must be an ImageFeatures")
            self._check_features(out, "encode_features(out=)")
            if isinstance(at, bool) or int(at) != at or at < 0 or at + len(images) > out.num_images:
                raise IndexError(f"encode_features: rows [{at}, {at + len(images)}) do not fit a bank of {out.num_images} images")
        feat = eng.encode_features(self._eng_images(*self._image_operand(images)))
        if out is None:
            return ImageFeatures(feat, self._feat_stamp(eng), self._handle)
        if tuple(feat.shape[1:]) != tuple(out._t.shape[1:]):
            raise RuntimeError(f"encode_features: these images give {tuple(feat.shape[1:])} features, the bank holds {tuple(out._t.shape[1:])}")
        out._t[int(at): int(at) + feat.shape[0]].copy_(feat)
        return out

    def features_from_tensor(self, t: torch.Tensor) -> "ImageFeatures":
        """Wrap a [U, Hf, Wf, 512] tensor in the compute dtype on the model's device (ImageFeatures.tensor() saved earlier, or an empty
        bank to fill with encode_features(out=)) as features of the image encoder AS IT IS NOW.  Shape, dtype and device are checked;
        that the values came from these weights is the caller's word."""
        if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[3] != self.image_encoder.output_channels:
            raise ValueError(f"features_from_tensor: expected a [U, Hf, Wf, {self.image_encoder.output_channels}] tensor, got "
                             + (f"shape {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__))
        if t.dtype != self.compute_dtype:
            raise ValueError(f"features_from_tensor: this model computes in {self.compute_dtype}, the tensor holds {t.dtype}")
        if t.device != self._flat.device:
            raise ValueError(f"features_from_tensor: the tensor is on {t.device}, the model on {self._flat.device}")
        if t.requires_grad:
            raise ValueError("features_from_tensor: cached features carry no gradient; pass t.detach()")
        return ImageFeatures(t.contiguous(), self._feat_stamp(self._ensure_engine()), self._handle)

    def _forward_features(self, features, token_ids, attention_mask, return_aux, image_index, grouped=False):
        """forward / forward_grouped over ImageFeatures: autograd through vqa_forward_features (gradients to the parameters outside
        the image encoder), otherwise the engine's no-tape routes."""
        eng = self._check_features(features, "forward")
        if not token_ids.is_cuda:
            raise RuntimeError("VQAModel (HIP) got CPU inputs; this implementation only runs on an MI355X (no CPU fallback)")
        feat = features._t
        dev = feat.device
        U, N = feat.shape[0], token_ids.shape[0]
        idx = self._image_index(image_index, U, N, dev)
        params = self._param_list()
        recording = torch.is_grad_enabled() and any(p.requires_grad for p in params)
        if recording and any(p.requires_grad for p in self._cnn_params()):
            raise RuntimeError("forward: ImageFeatures stand in for a frozen image encoder: call model.image_encoder.requires_grad_(False)")
        if return_aux and recording:
            raise NotImplementedError("forward(ImageFeatures, return_aux=True) under autograd: gradients through aux outputs are not "
                                      "supported from cached features (run it under torch.no_grad())")
        token_ids = token_ids.contiguous().long()
        maskf = None if attention_mask is None else attention_mask.contiguous().float()
        grouped = grouped or image_index is not None
        if idx is None and (grouped or U != N):
            idx = self._implied_index(U, N, dev)
        if recording:
            flat = _FlatParams.apply(self._flat, self._handle, *params)
            self._pending_plan = self._finetune_plan(params, False, self.training)
            logits = torch.ops.vqa_hip.vqa_forward_features(feat, token_ids, maskf, idx, flat, self._handle, self.training)
            return logits, None
        if grouped and not self.training:
            # eval with an image index: the images route is answer(encode_images(images)); so is this one, from the features
            logits, aux = eng.answer(eng.context_from_features(feat, want_aux=return_aux), token_ids, maskf, idx, want_aux=return_aux)
            return (logits, aux) if return_aux else (logits, None)
        logits, aux, _ = eng.forward_features(feat, token_ids, maskf, self.training, return_aux, need_tape=False, kv_index=idx,
                                              plan=self._modes_plan())
        return (logits, aux) if return_aux else (logits, None)

    def _inference_only(self, what, images=None):
        if self.training:
            raise RuntimeError(f"{what} is inference only: call model.eval() first")
        if torch.is_grad_enabled() and ((images is not None and images.requires_grad)
                                        or any(p.requires_grad for p in self._param_list())):
            raise RuntimeError(f"{what} is inference only: run it under torch.no_grad() (or freeze the parameters)")

    def _image_index(self, image_index, U: int, N: int, dev):
        """int32 [N] device copy of a checked index, or None for the implied one (i -> i when N == U, every question on image 0 when
        U == 1).  Range check: free for a CPU index, one device-to-host read for a device index."""
        if image_index is None:
            if N == U or U == 1:
                return None
            raise ValueError(f"image_index=None needs as many questions as images or one image; got {N} questions, {U} images")
        if not isinstance(image_index, torch.Tensor):
            image_index = torch.as_tensor(image_index)
        if image_index.dim() != 1 or image_index.shape[0] != N:
            raise ValueError(f"image_index must be 1-D with one entry per question ({N}); got shape {tuple(image_index.shape)}")
        if image_index.dtype.is_floating_point or image_index.dtype.is_complex or image_index.dtype == torch.bool:
            raise ValueError(f"image_index must hold integers, got {image_index.dtype}")
        if N:
            lo, hi = (int(v) for v in torch.stack(torch.aminmax(image_index)).tolist())
            if lo < 0 or hi >= U:
                raise IndexError(f"image_index holds {lo if lo < 0 else hi}, outside [0, {U}) for {U} images")
        return image_index.to(device=dev, dtype=torch.int32)

    def _implied_index(self, U: int, N: int, dev):
        return torch.arange(N, device=dev, dtype=torch.int32) if U == N else torch.zeros(N, device=dev, dtype=torch.int32)

    def _graph_put(self, key, g):
        if len(self._graphs) >= self.graph_max_shapes:
            torch.cuda.synchronize()                 # an evicted graph's private pool must outlive its last replay in flight
            while len(self._graphs) >= self.graph_max_shapes:
                self._graphs.pop(next(iter(self._graphs)))
        self._graphs[key] = g

    def _capture(self, fn):
        """fn() twice on a side stream (warm-up), then captured into a HIP graph; returns (graph, fn's output in the graph's pool)."""
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = fn()
        return graph, out

    def _forward_indexed(self, images, token_ids, attention_mask, return_aux, image_index):
        self._inference_only("forward(image_index=...)", images)
        eng = self._ensure_engine()
        images, norm = self._image_operand(images)
        token_ids = token_ids.contiguous().long()
        U, N = images.shape[0], token_ids.shape[0]
        idx = self._image_index(image_index, U, N, images.device)
        if idx is None:
            idx = self._implied_index(U, N, images.device)
        maskf = None if attention_mask is None else attention_mask.contiguous().float()
        if (self.graph_inference and not return_aux and 0 < N <= self.graph_max_batch and not torch.cuda.is_current_stream_capturing()):
            key = ("image_index", tuple(images.shape), tuple(token_ids.shape), maskf is not None, self._flat.data_ptr(), eng.fold_eval,
                   eng.fuse_stem_eval, self._infer_precision) + (() if norm is None else (norm,))
            g = self._graphs.pop(key, None)
            if g is None:
                st_img, st_ids, st_idx = images.detach().clone(), token_ids.detach().clone(), idx.clone()
                st_msk = None if maskf is None else maskf.detach().clone()
                graph, out = self._capture(lambda: eng.answer(eng.encode_images(self._eng_images(st_img, norm)), st_ids, st_msk, st_idx)[0])
                g = (graph, st_img, st_ids, st_msk, st_idx, out)
            self._graph_put(key, g)                  # (re)inserted at the young end of the LRU order
            graph, st_img, st_ids, st_msk, st_idx, out = g
            st_img.copy_(images); st_ids.copy_(token_ids); st_idx.copy_(idx)
            if st_msk is not None:
                st_msk.copy_(maskf)
            graph.replay()
            return out.clone(), None
        logits, aux = eng.answer(eng.encode_images(self._eng_images(images, norm), want_aux=return_aux), token_ids, maskf, idx, want_aux=return_aux)
        return (logits, aux) if return_aux else (logits, None)

    def forward_grouped(self, images: torch.Tensor, token_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                        image_index: Optional[torch.Tensor] = None, return_aux: bool = False) -> Tuple[torch.Tensor, Optional[Dict]]:
        """Many questions per image, training included: images [U, 3, H, W], token_ids / attention_mask [N, L], question i is asked of
        image image_index[i] (None: the rules of answer()).  Computes
            feat = image_encoder(images)            one CNN batch of the U images: train-mode BatchNorm statistics over U images,
                                                    running statistics updated once from them
            img  = image_projector(feat)            projector dropout drawn per image token (U rows)
            text = text_encoder(token_ids, mask)    per question
            cross-attention layer l: query batch i attends to norm_kv(img)[image_index[i]] (attention dropout per question)
            pools, gate, output norm, answer head   per question
        With dropout 0 this is fusion(image_encoder(images)[image_index], text, ...).  Gradients reach the parameters and, when
        images.requires_grad, the images ([U, 3, H, W]); an image without a question still counts in the BatchNorm statistics and gets
        a zero feature gradient.  With U = N and image_index = arange(N) every value (dropout included) is bit-equal to forward().
        Eval mode without autograd delegates to forward(image_index=...).  return_aux=True raises NotImplementedError while autograd
        records (no gradients through aux under grouping); otherwise aux has U image rows and N question rows.
        Raises IndexError for an index outside [0, U), ValueError for a wrong shape or dtype.
        images may be an ImageFeatures of the U images (encode_features; frozen, eval-mode image encoder): the CNN pass is skipped."""
        if isinstance(images, ImageFeatures):
            return self._forward_features(images, token_ids, attention_mask, return_aux, image_index, grouped=True)
        if not images.is_cuda:
            raise RuntimeError("VQAModel (HIP) got CPU inputs; this implementation only runs on an MI355X (no CPU fallback)")
        U, N = len(images), token_ids.shape[0]
        idx = self._image_index(image_index, U, N, images.device)
        params = self._param_list()
        recording = torch.is_grad_enabled() and (images.requires_grad or any(p.requires_grad for p in params))
        if return_aux and recording:
            raise NotImplementedError("forward_grouped(return_aux=True) under autograd: gradients through aux outputs are not supported "
                                      "with an image index (run it under torch.no_grad())")
        if not self.training and not recording:
            return self.forward(images, token_ids, attention_mask, return_aux=return_aux, image_index=image_index)
        eng = self._ensure_engine()
        images, norm = self._image_operand(images)
        token_ids = token_ids.contiguous().long()
        maskf = None if attention_mask is None else attention_mask.contiguous().float()
        if idx is None:
            idx = self._implied_index(U, N, images.device)
        if recording:
            self._byte_norm = norm
            flat = _FlatParams.apply(self._flat, self._handle, *params) if any(p.requires_grad for p in params) else self._flat
            self._pending_plan = self._finetune_plan(params, images.requires_grad, self.training)
            logits = torch.ops.vqa_hip.vqa_forward_grouped(images, token_ids, maskf, idx, flat, self._handle, self.training)
            return logits, None
        logits, aux, _ = eng.forward(self._eng_images(images, norm), token_ids, maskf, self.training, return_aux, need_tape=False, kv_index=idx,
                                     plan=self._modes_plan())
        return (logits, aux) if return_aux else (logits, None)

    def encode_images(self, images: torch.Tensor) -> ImageContext:
        """Run the image half of the eval forward once per image (stem, residual stages, SE / spatial attention, projector and the
        K / V projections of every cross-attention layer) and keep it for answer().  Inference only (eval mode, no autograd).  The
        context keeps about 100 KB per image at the default configuration (49 tokens x 2 layers x K | V in bf16), and the NHWC features
        plus projected tokens for return_aux (another ~75 KB).
        images may be an ImageFeatures (encode_features): only the projector and the K / V projections run."""
        if isinstance(images, ImageFeatures):
            self._inference_only("encode_images")
            eng = self._check_features(images, "encode_images")
            return ImageContext(images.num_images, eng.context_from_features(images._t, want_aux=True), self._ctx_stamp(eng), self._handle)
        if not images.is_cuda:
            raise RuntimeError("VQAModel (HIP) got CPU inputs; this implementation only runs on an MI355X (no CPU fallback)")
        self._inference_only("encode_images", images)
        eng = self._ensure_engine()
        ctx = eng.encode_images(self._eng_images(*self._image_operand(images)), want_aux=True)
        return ImageContext(len(images), ctx, self._ctx_stamp(eng), self._handle)

    def answer(self, context: ImageContext, token_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
               image_index: Optional[torch.Tensor] = None, return_aux: bool = False) -> Tuple[torch.Tensor, Optional[Dict]]:
        """Logits of N questions over a context of encode_images(): question i is asked of image image_index[i] (None: i -> i when
        N == context.num_images, or every question on image 0 when the context holds one image).  Equals forward(images[image_index],
        token_ids, attention_mask) and costs only the question path.  Inference only.  Up to graph_max_batch questions (without aux) a
        captured HIP graph of the question path is replayed, keyed on (images, questions, length, mask, parameters, precision); the
        context's K / V are copied into the graph's buffers, so one graph serves every context of that shape.  A device image_index
        costs one device-to-host read (the range check); a CPU one costs none.  Raises RuntimeError for a context made before the
        parameters, BatchNorm buffers (load_state_dict) or inference precision changed, or before a train-mode forward."""
        if not isinstance(context, ImageContext) or context._handle != self._handle:
            raise ValueError("answer() needs an ImageContext made by this model's encode_images()")
        self._inference_only("answer")
        eng = self._ensure_engine()
        if context._stamp != self._ctx_stamp(eng):
            raise RuntimeError("stale ImageContext: the parameters, BatchNorm buffers or inference precision changed since "
                               "encode_images() made it; encode the images again")
        if not token_ids.is_cuda:
            raise RuntimeError("VQAModel (HIP) got CPU inputs; this implementation only runs on an MI355X (no CPU fallback)")
        token_ids = token_ids.contiguous().long()
        U, (N, L) = context.num_images, token_ids.shape
        dev = token_ids.device
        idx = self._image_index(image_index, U, N, dev)
        maskf = None if attention_mask is None else attention_mask.contiguous().float()
        ec = context._eng
        if (self.graph_inference and not return_aux and 0 < N <= self.graph_max_batch and not torch.cuda.is_current_stream_capturing()):
            key = ("answer", U, N, L, maskf is not None, idx is None, self._flat.data_ptr(), self._infer_precision)
            g = self._graphs.pop(key, None)
            if g is None:
                st_ids = token_ids.clone()
                st_msk = None if maskf is None else maskf.clone()
                st_idx = self._implied_index(U, N, dev) if idx is None else idx.clone()
                st_ctx = {"kv": ec["kv"].clone(), "U": U, "ntok": ec["ntok"]}
                graph, out = self._capture(lambda: eng.answer(st_ctx, st_ids, st_msk, st_idx)[0])
                g = (graph, st_ctx, st_ids, st_msk, st_idx, out)
            self._graph_put(key, g)
            graph, st_ctx, st_ids, st_msk, st_idx, out = g
            st_ctx["kv"].copy_(ec["kv"]); st_ids.copy_(token_ids)
            if idx is not None:
                st_idx.copy_(idx)
            if st_msk is not None:
                st_msk.copy_(maskf)
            graph.replay()
            return out.clone(), None
        if idx is None:
            idx = self._implied_index(U, N, dev)
        logits, aux = eng.answer(ec, token_ids, maskf, idx, want_aux=return_aux)
        return (logits, aux) if return_aux else (logits, None)

    # ---- top-k answers with probabilities (extension, inference only)
    def _topk_args(self, top_k, answer_mask, temperature, N: int, dev):
        """Checked (k, mask | None, scale = fp32(1 / temperature)) of predict_topk / answer_topk; ValueError for what they refuse."""
        A = self.num_answers
        if isinstance(top_k, bool) or not isinstance(top_k, int) or not 1 <= top_k <= min(64, A):
            raise ValueError(f"top_k must be an integer in 1 ... {min(64, A)}, got {top_k!r}")
        try:
            t = float(temperature)
        except (TypeError, ValueError):
            raise ValueError(f"temperature must be a positive finite number, got {temperature!r}") from None
        scale = torch.tensor(1.0 / t, dtype=torch.float32).item() if (math.isfinite(t) and t > 0.0) else 0.0
        if not (math.isfinite(scale) and scale > 0.0):
            raise ValueError(f"temperature must be finite and > 0 (with 1 / temperature a positive finite float32), got {temperature!r}")
        if answer_mask is not None:
            if (not isinstance(answer_mask, torch.Tensor) or answer_mask.dtype not in (torch.bool, torch.uint8)
                    or tuple(answer_mask.shape) not in ((A,), (N, A))):
                raise ValueError(f"answer_mask must be a bool or uint8 tensor of shape [{A}] or [{N}, {A}], got "
                                 + (f"{answer_mask.dtype} {tuple(answer_mask.shape)}" if isinstance(answer_mask, torch.Tensor)
                                    else type(answer_mask).__name__))
            if answer_mask.device != dev:
                raise ValueError(f"answer_mask must be on the model's device ({dev}), got {answer_mask.device}")
            answer_mask = answer_mask.contiguous()
        return top_k, answer_mask, scale

    def _topk_route(self, base_key, N, init, feed, logits_fn, k, mask, scale, want):
        """logits_fn(*inputs) (logits in the compute dtype), then vqa_softmax_topk.  Up to graph_max_batch rows both are ONE captured
        graph, keyed on base_key + ("topk", k, mask shape, scale, want): init() makes the static inputs on a miss, feed (None = keep
        what was captured) is copied into them, and copies of the static outputs are returned.  Larger batches: the same two steps
        eagerly on feed.  The scale is part of the key (it is a launch argument frozen into the graph), so every new temperature is a
        capture, and these graphs share the graph_max_shapes LRU with those of forward() / answer()."""
        tk = self._pkg.kernels.softmax_topk

        def tail(lg, msk):
            idx, probs, lf = tk(lg, k, msk, scale, want_logits=want and lg.dtype != torch.float32)
            return lg, idx, probs, lf

        if self.graph_inference and 0 < N <= self.graph_max_batch and not torch.cuda.is_current_stream_capturing():
            key = base_key + ("topk", k, None if mask is None else tuple(mask.shape), float(scale), bool(want))
            g = self._graphs.pop(key, None)
            fresh = g is None
            if fresh:
                st = init()                          # (clones of feed: nothing to copy in before this first replay)
                st_mask = None if mask is None else mask.clone()
                graph, out = self._capture(lambda: tail(logits_fn(*st), st_mask))
                g = (graph, st, st_mask, out)
            self._graph_put(key, g)                  # (re)inserted at the young end of the LRU order
            graph, st, st_mask, (lg, idx, probs, lf) = g
            if not fresh:
                for s_, t in zip(st, feed):
                    if t is not None:
                        s_.copy_(t)
                if st_mask is not None:
                    st_mask.copy_(mask)
            graph.replay()
            return TopK(idx.clone(), probs.clone(), (lg if lf is None else lf).clone() if want else None)
        lg, idx, probs, lf = tail(logits_fn(*feed), mask)
        return TopK(idx, probs, (lg if lf is None else lf) if want else None)

    def predict_topk(self, images: torch.Tensor, token_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, top_k: int = 5,
                     image_index: Optional[torch.Tensor] = None, answer_mask: Optional[torch.Tensor] = None, temperature: float = 1.0,
                     return_logits: bool = False) -> TopK:
        """The top_k best answers of every question with their probabilities: kernels.softmax_topk(forward(...)[0], top_k, answer_mask,
        1 / temperature) bit for bit, with the forward and the top-k launch in one captured HIP graph up to graph_max_batch questions
        (keyed on the shapes, top_k, the mask's shape, the temperature and return_logits).  Inference only: eval mode (it is NOT set
        for the caller: train mode raises RuntimeError), no autograd; image_index as in forward().  answer_mask: bool / uint8
        [num_answers] or [N, num_answers] on the model's device, True = the answer may be given; a row with fewer than top_k allowed
        answers ends with not-allowed ones at probability 0 (lowest index first), a row with none (or an all-padding question, whose
        logits are NaN) gets NaN probabilities and indices 0 ... top_k-1.  Ties go to the lower index.  ValueError for top_k outside
        1 ... min(64, num_answers), a temperature that is not finite and > 0, or a mask of another shape / dtype / device.
        Keep to a few fixed temperatures on the graphed route: each distinct (top_k, mask shape, temperature, return_logits) is a graph
        of its own -- two warm-up forwards, a capture and static copies of the inputs on first use -- in the same graph_max_shapes-entry
        LRU as the graphs of forward() / answer(), which a stream of new values would evict.  A per-request temperature belongs on the
        eager route (graph_inference = False, or kernels.softmax_topk on forward()'s logits)."""
        if not images.is_cuda:
            raise RuntimeError("VQAModel (HIP) got CPU inputs; this implementation only runs on an MI355X (no CPU fallback)")
        self._inference_only("predict_topk", images)
        eng = self._ensure_engine()
        images, norm = self._image_operand(images)
        nkey = () if norm is None else (norm,)
        token_ids = token_ids.contiguous().long()
        maskf = None if attention_mask is None else attention_mask.contiguous().float()
        U, N = images.shape[0], token_ids.shape[0]
        if image_index is None:
            k, amask, scale = self._topk_args(top_k, answer_mask, temperature, U, images.device)
            key = (tuple(images.shape), tuple(token_ids.shape), maskf is not None, self._flat.data_ptr(), eng.fold_eval,
                   getattr(eng, "fuse_stem_eval", None), self._infer_precision) + nkey
            feed = [images, token_ids, maskf]
            graphed = self.graph_inference and 0 < U <= self.graph_max_batch and not torch.cuda.is_current_stream_capturing()
            plan = None if graphed else self._modes_plan()           # (forward()'s two eval routes)
            fn = lambda x, ids, msk: eng.forward(self._eng_images(x, norm), ids, msk, False, False, need_tape=False, lowp_logits=True, plan=plan)[0]
            return self._topk_route(key, U, lambda: [None if t is None else t.detach().clone() for t in feed], feed, fn,
                                    k, amask, scale, return_logits)
        idx = self._image_index(image_index, U, N, images.device)
        if idx is None:
            idx = self._implied_index(U, N, images.device)
        k, amask, scale = self._topk_args(top_k, answer_mask, temperature, N, images.device)
        key = ("image_index", tuple(images.shape), tuple(token_ids.shape), maskf is not None, self._flat.data_ptr(), eng.fold_eval,
               eng.fuse_stem_eval, self._infer_precision) + nkey
        feed = [images, token_ids, maskf, idx]
        fn = lambda x, ids, msk, ix: eng.answer(eng.encode_images(self._eng_images(x, norm)), ids, msk, ix, lowp_logits=True)[0]
        return self._topk_route(key, N, lambda: [None if t is None else t.detach().clone() for t in feed], feed, fn,
                                k, amask, scale, return_logits)

    def answer_topk(self, context: ImageContext, token_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, top_k: int = 5,
                    image_index: Optional[torch.Tensor] = None, answer_mask: Optional[torch.Tensor] = None, temperature: float = 1.0,
                    return_logits: bool = False) -> TopK:
        """predict_topk over a context of encode_images(): kernels.softmax_topk(answer(context, ...)[0], ...) bit for bit, the question
        path and the top-k launch in one captured graph up to graph_max_batch questions.  The rules of answer() (inference only, a
        stale context raises RuntimeError) and the arguments of predict_topk()."""
        if not isinstance(context, ImageContext) or context._handle != self._handle:
            raise ValueError("answer_topk() needs an ImageContext made by this model's encode_images()")
        self._inference_only("answer_topk")
        eng = self._ensure_engine()
        if context._stamp != self._ctx_stamp(eng):
            raise RuntimeError("stale ImageContext: the parameters, BatchNorm buffers or inference precision changed since "
                               "encode_images() made it; encode the images again")
        if not token_ids.is_cuda:
            raise RuntimeError("VQAModel (HIP) got CPU inputs; this implementation only runs on an MI355X (no CPU fallback)")
        token_ids = token_ids.contiguous().long()
        U, (N, L) = context.num_images, token_ids.shape
        dev = token_ids.device
        idx = self._image_index(image_index, U, N, dev)
        maskf = None if attention_mask is None else attention_mask.contiguous().float()
        k, amask, scale = self._topk_args(top_k, answer_mask, temperature, N, dev)
        ec = context._eng
        key = ("answer", U, N, L, maskf is not None, idx is None, self._flat.data_ptr(), self._infer_precision)
        ntok = ec["ntok"]
        fn = lambda kv, ids, msk, ix: eng.answer({"kv": kv, "U": U, "ntok": ntok}, ids, msk, ix, lowp_logits=True)[0]

        def init():
            return [ec["kv"].clone(), token_ids.clone(), None if maskf is None else maskf.clone(),
                    self._implied_index(U, N, dev) if idx is None else idx.clone()]

        graphed = self.graph_inference and 0 < N <= self.graph_max_batch and not torch.cuda.is_current_stream_capturing()
        feed = [ec["kv"], token_ids, maskf, idx if (graphed or idx is not None) else self._implied_index(U, N, dev)]
        return self._topk_route(key, N, init, feed, fn, k, amask, scale, return_logits)

    # ---- explaining an answer (extension, inference only)
    def explain(self, images, token_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, answers: Optional[torch.Tensor] = None,
                methods=EXPLAIN_METHODS, normalize: bool = True) -> Explanation:
        """Where the model looked, per question, on the image-feature grid (7 x 7 at 224 x 224):
          "gradcam"    Grad-CAM of the image features for the explained class c: relu(sum_k alpha_k * feat_k) with alpha_k the spatial
                       mean of d logits[:, c] / d feat_k.  The backward of that one score stops at the image features: no weight
                       gradient, no gradient buffer, no CNN or text-encoder backward (HipEngine.explain_route).
          "attention"  the cross-attention probabilities, mean over layers, heads and the question's real tokens: the reference's
                       get_attention_visualization averaged over the question.  Each map sums to 1 before normalisation; an
                       all-padding question gives NaN, as its logits are.  ValueError for a model without cross-attention layers.
        answers: int64 [N] (any integer dtype, CPU or device) -- the class to explain per question -- or None for the arg-max of this
        call's own logits (ties to the lower index).  Range-checked as an image index is: free for a CPU tensor, one device-to-host
        read for a device tensor; IndexError outside [0, num_answers).  normalize: each map divided by its maximum (a map that is all
        zero stays zero).  images: float NCHW or a ByteImages (the same result bit for bit).
        Inference only: train mode raises RuntimeError (eval mode is NOT set for the caller); it runs with and without
        torch.no_grad() and never touches autograd, parameters' .grad, BatchNorm buffers, dropout seeds or a trainer's state, so it
        may be called between two training steps.  The logits are the eval-mode TAPED forward's (what model(...) gives under
        autograd in eval mode), not the Conv+BN-folded inference path's; in bf16 the two differ by rounding.  Eager: not captured.
        ValueError for unknown or empty methods, or answers of another shape or dtype, before anything is launched."""
        if isinstance(methods, str):
            methods = (methods,)
        methods = tuple(methods)
        if not methods or any(m not in EXPLAIN_METHODS for m in methods) or len(set(methods)) != len(methods):
            raise ValueError(f"explain: methods must be a non-empty selection of {EXPLAIN_METHODS}, got {methods!r}")
        if isinstance(images, ImageFeatures):
            raise TypeError("explain: takes images (float NCHW or ByteImages), not ImageFeatures")
        N = token_ids.shape[0]
        n_img = images.shape_nchw[0] if _is_bytes(images) else images.shape[0]
        if token_ids.dim() != 2 or n_img != N:
            raise ValueError(f"explain: one question [N, L] per image expected; got {n_img} images and token_ids {tuple(token_ids.shape)}")
        if answers is not None:
            if not isinstance(answers, torch.Tensor):
                answers = torch.as_tensor(answers)
            if answers.dim() != 1 or answers.shape[0] != N:
                raise ValueError(f"explain: answers must be 1-D with one class per question ({N}); got shape {tuple(answers.shape)}")
            answers = _checked_index(answers, self.num_answers, "explain: answers")
        if "attention" in methods and not self.config["num_cross_layers"]:
            raise ValueError("explain: \"attention\" needs a model with cross-attention layers (num_cross_layers = 0)")
        if self.training or any(self._part_modes()):
            raise RuntimeError("explain is inference only: call model.eval() first (every part in eval mode)")
        if not (images.data if _is_bytes(images) else images).is_cuda or not token_ids.is_cuda:
            raise RuntimeError("VQAModel (HIP) got CPU inputs; this implementation only runs on an MI355X (no CPU path)")
        eng = self._ensure_engine()
        K = self._pkg.kernels
        with torch.no_grad():
            images, norm = self._image_operand(images)
            dev = images.device
            token_ids = token_ids.contiguous().long()
            maskf = None if attention_mask is None else attention_mask.contiguous().float()
            if answers is not None:
                answers = answers.to(device=dev, dtype=torch.int64).contiguous()
            plan = self.__dict__.get("_explain_plan")
            if plan is None:
                plan = self.__dict__["_explain_plan"] = self._pkg.finetune.explain_plan(self._param_entries)
            r = eng.explain_route(self._eng_images(images.detach(), norm), token_ids, maskf, plan, class_ids=answers,
                                  want_dfeat="gradcam" in methods, want_caw="attention" in methods)
            Hf, Wf, Cf = r["Hf"], r["Wf"], r["Cf"]
            logits = r["logits"] if r["logits"].dtype == torch.float32 else r["logits"].float()
            cam = att = None
            if "gradcam" in methods:
                cam = K.gradcam(r["feat"], r["dfeat"], N, Hf * Wf, Cf, normalize=normalize).view(N, Hf, Wf)
            if "attention" in methods:
                att = K.attention_map(r["caw"], maskf, normalize=normalize).view(N, Hf, Wf)
        return Explanation(logits, r["chosen"], cam, att)

    graph_inference = True        # eval-mode no-grad forward()/predict() replay a captured HIP graph up to graph_max_batch
    graph_max_batch = 64          # (the serving case, api/inference.py:196-323: model(...) at B = 1 ... a few)
    graph_max_shapes = 16         # distinct input shapes kept captured (least recently used dropped first)
    max_live_tapes = 4            # training forwards whose backward has not run yet (each pins its activations)

    def predict(self, images, token_ids, attention_mask=None, top_k: int = 5, image_index=None):
        self.eval()
        with torch.no_grad():
            logits, _ = self.forward(images, token_ids, attention_mask, image_index=image_index)    # (replays the HIP graph of this shape for B <= graph_max_batch)
            probs = F.softmax(logits, dim=-1)
            top_probs, top_indices = probs.topk(top_k, dim=-1)
        return top_indices, top_probs

    def _attention_visualization(self, attention_weights: list, spatial_size: int = 7) -> torch.Tensor:
        avg = torch.stack(attention_weights, dim=0).mean(dim=0).mean(dim=1)
        b, lq, _ = avg.shape
        return avg.view(b, lq, spatial_size, spatial_size)

    def get_attention_maps(self, images, token_ids, attention_mask=None, image_index=None) -> Dict[str, torch.Tensor]:
        _, aux = self.forward(images, token_ids, attention_mask, return_aux=True, image_index=image_index)
        vis = self._attention_visualization(aux["cross_attention_weights"], self.image_encoder.output_spatial_size)
        return {"cross_attention": aux["cross_attention_weights"], "cross_attention_spatial": vis}

    def get_num_parameters(self) -> Dict[str, int]:
        counts = {k: sum(p.numel() for p in getattr(self, k).parameters())
                  for k in ("image_encoder", "text_encoder", "fusion", "answer_head")}
        counts["total"] = sum(counts.values())
        return counts


def group_by_image(image_ids) -> Tuple[torch.Tensor, torch.Tensor]:
    """Grouped form of a batch that carries each sample's image id (the reference dataset's sample info `image_id`):
    returns (first, image_index), both int64.  `first` holds the batch position of the first occurrence of each distinct image, in
    order of appearance; image_index[i] is the position in `first` of sample i's image.  So images[first] with image_index is what
    forward_grouped / HipTrainer.step(image_index=) take, and images[first][image_index] equals images when samples of one image
    carry the same image.  A tensor argument keeps its device."""
    dev = image_ids.device if isinstance(image_ids, torch.Tensor) else torch.device("cpu")
    ids = image_ids.tolist() if isinstance(image_ids, torch.Tensor) else list(image_ids)
    slot: Dict[Any, int] = {}
    first: List[int] = []
    index: List[int] = []
    for i, key in enumerate(ids):
        if key not in slot:
            slot[key] = len(first)
            first.append(i)
        index.append(slot[key])
    return (torch.tensor(first, dtype=torch.long, device=dev), torch.tensor(index, dtype=torch.long, device=dev))


def getattr_path(obj, dotted: str):
    for part in dotted.split("."):
        obj = getattr(obj, part)
    return obj


def create_vqa_model(vocab_size: int = 10000, num_answers: int = 1000, use_attention: bool = True, **kwargs) -> VQAModel:
    return VQAModel(vocab_size=vocab_size, num_answers=num_answers, use_se_attention=use_attention,
                    use_spatial_attention=use_attention, **kwargs)


def load_vqa_model(checkpoint_path: str, device: str = "cpu") -> VQAModel:
    # the checkpoint dict of training/train.py:280-288 holds tensors, a config dict and scalars only: the weights-only loader
    # (executes nothing from the file) reads it
    checkpoint = torch.load(checkpoint_path, map_location=device, weights_only=True)
    model = VQAModel(**checkpoint.get("config", {}))
    model.load_state_dict(checkpoint["model_state_dict"])
    return model.to(device)
