"""Host side of the captured train step (HipTrainer.step_graphed): the self-describing dropout seed word, the device step-state
block as ctypes sees it, and the key a captured graph is filed under.  Pure host logic (no GPU, no library): tests/test_step_graph_cpu.py.

A captured launch freezes its by-value arguments.  The dropout seeds and AdamW's hyper-parameters are such arguments, so a captured
step reads them from one device block instead (include/vqa_hip.h, vqa_step_state), which vqa_step_state_set rewrites before every
replay.  The seed word tells the kernels which form they were given (csrc/common.h, drop_resolve):
    bit 63 clear    the seed itself: rank << 44 | (seed_base + step_id) << 12 | site -- the rank sits at bit 44, so this form never
                    reaches bit 63 and every seed handed out before this format existed still means what it meant;
    bit 63 set      bits 0-47: device address of vqa_step_state.seed_step, bits 48-59: the site; the seed is *address | site.
"""
from __future__ import annotations

import ctypes as C

SEED_INDIRECT = 1 << 63
ADDR_BITS = 48
SITE_BITS = 12
STEP_MASK = 0xFFFFFFFF


def seed_step(rank: int, seed_base: int, step_id: int) -> int:
    """The per-step half of a seed (what vqa_step_state.seed_step holds): the site bits are zero."""
    return (int(rank) << 44) | (((int(seed_base) + int(step_id)) & STEP_MASK) << SITE_BITS)


def plain_seed(rank: int, seed_base: int, step_id: int, site: int) -> int:
    """The by-value seed of HipEngine._seed()."""
    return seed_step(rank, seed_base, step_id) | int(site)


def seed_word(addr: int, site: int) -> int:
    """The flagged seed word: `addr` is the device address of a vqa_step_state.seed_step."""
    addr, site = int(addr), int(site)
    if not 0 < addr < (1 << ADDR_BITS) or addr & 7:
        raise ValueError(f"seed word: the device address {addr:#x} must be 8-byte aligned and below 2^{ADDR_BITS}")
    if not 0 <= site < (1 << SITE_BITS):
        raise ValueError(f"seed word: site {site} does not fit {SITE_BITS} bits")
    return SEED_INDIRECT | (site << ADDR_BITS) | addr


def is_indirect(word: int) -> bool:
    return bool(int(word) & SEED_INDIRECT)


def decode_seed_word(word: int):
    """(address, site) of a flagged seed word."""
    word = int(word)
    if not word & SEED_INDIRECT:
        raise ValueError("not a flagged seed word")
    return word & ((1 << ADDR_BITS) - 1), (word >> ADDR_BITS) & ((1 << SITE_BITS) - 1)


def resolve(word: int, read) -> int:
    """Python model of drop_resolve (csrc/common.h): read(address) returns the 64-bit word stored there."""
    word = int(word)
    if not word & SEED_INDIRECT:
        return word
    addr, site = decode_seed_word(word)
    return int(read(addr)) | site


class StepState(C.Structure):
    """vqa_step_state of include/vqa_hip.h (16-byte aligned, 64 bytes)."""
    _fields_ = [("calls", C.c_longlong), ("seed_step", C.c_ulonglong),
                ("lr", C.c_float), ("b1", C.c_float), ("b2", C.c_float), ("eps", C.c_float), ("wd", C.c_float),
                ("max_norm", C.c_float), ("gscale", C.c_float), ("ema_decay", C.c_float), ("ema_warmup", C.c_int),
                ("_pad", C.c_int * 3)]


GROUPS_MAX = 16


class GroupHyper(C.Structure):
    """vqa_group_hyper of include/vqa_hip.h (16-byte aligned, 128 bytes): the parameter groups' lr scales and weight decays."""
    _fields_ = [("lr_scale", C.c_float * GROUPS_MAX), ("wd", C.c_float * GROUPS_MAX)]


GROUP_HYPER_BYTES = 128


STATE_BYTES = 64
SEED_STEP_OFFSET = 8


def table_id(generation, groups=None, guard=False):
    """step_key's table_id: the generation of the optimizer's range table (None: the plain kernels), and with parameter groups their
    STRUCTURE beside it (finetune.ParamGroups.key(): the group of every parameter) -- a grouped step issues other launches, and the
    per-range group array is rebuilt with the table.  The groups' VALUES (lr_scale, weight_decay) live in a device block and never
    enter: changing them captures nothing anew.
    guard: the trainer runs the non-finite guard (HipTrainer(nonfinite=...)): the step then takes its norm from other entries, hands
    AdamW another skip word and saves / restores the BatchNorm buffers around a train-mode CNN -- the flag enters step_key here,
    with the rest of what decides the optimizer tail's launches, as ("guard", the id without it)."""
    tid = generation if groups is None else (generation, tuple(groups))
    return ("guard", tid) if guard else tid


def _sig(t):
    """Shape and dtype of a tensor (None stays None)."""
    return None if t is None else (tuple(t.shape), str(t.dtype))


def step_key(*, features: bool, images, token_ids, attention_mask, image_index, targets, plan, loss_kind: str, loss_opts,
             ema: bool, metrics, flat_ptr: int, wsrc_ptr: int, table_id):
    """What a captured train step is filed under: everything that decides WHICH launches the step issues, with which sizes and on
    which buffers -- and nothing that only decides values (the tensors' contents, lr, betas, eps, weight decay, max_norm, the EMA
    decay and warm-up flag, the step number: those reach the graph through its static inputs and the state block).
    images / token_ids / attention_mask / image_index: tensors or None (shape and dtype enter; the mask and the index also by presence);
    images may be a ByteImages: its data's shape and dtype and its mean / std enter (the lookup table is baked into the graph);
    targets: a label tensor, or SoftTargets (ids / weights / counts: K and whether counts ride along);
    plan: finetune.Plan or None (trainable tuple and modes); loss_opts: (label_smoothing, ignore_index, id of the class-weight buffer);
    metrics: the tracker object or None (its identity: the graph writes that object's device counters);
    flat_ptr / wsrc_ptr: addresses of the parameter buffer and of the bf16 operand copy; table_id: generation of the optimizer's range
    table (None: the plain kernels) -- a generation, not an address: a rebuilt table may land on the address of the one it replaced,
    with other sizes, and a graph captured on the old one must never be found again.  (The engine's buffer of packed backward
    operands is re-laid when a new trainable set needs more of them; step_graphed checks its generation when it finds a graph.)
    With parameter groups table_id is what table_id() below makes of the generation and the groups' structure."""
    if hasattr(targets, "ids") and hasattr(targets, "weights"):
        tsig = ("soft", _sig(targets.ids), _sig(targets.weights), _sig(getattr(targets, "counts", None)))
    else:
        tsig = ("hard", _sig(targets))
    if hasattr(images, "shape_nchw"):             # ByteImages: the graph's table is the one of this mean / std
        images_sig = ("bytes", _sig(images.data), tuple(images.mean), tuple(images.std))
    else:
        images_sig = _sig(images)
    return ("features" if features else "images", images_sig, _sig(token_ids), _sig(attention_mask), _sig(image_index), tsig,
            None if plan is None else (tuple(plan.trainable), tuple(plan.modes)), str(loss_kind), loss_opts, bool(ema),
            None if metrics is None else id(metrics), int(flat_ptr), int(wsrc_ptr), table_id)
