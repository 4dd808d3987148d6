"""GPU: HipEngine.forward, encode_images and answer issue, launch for launch and argument for argument, what they issued before
they were composed from one set of forward parts (engine.py: _stem_fwd, _stages_fwd, _text_fwd, _projector_fwd, _cross_kv_path,
_cross_layers_fwd, _tail_fwd, _aux_of).

tests/golden/forward_launches.json holds the ordered launch list of every route below.  It was WRITTEN AT THE PARENT of the commit
that introduced those parts (the three routes were still three hand-kept copies there), so it is the old code's behaviour, not
this code's.  Regenerate it only when a change is MEANT to alter what a route launches, on an MI355X, from the commit whose
launches are to become the reference:

    python tests/test_gpu_forward_launches.py --write

An entry is the C-ABI entry point's name followed by every argument `_lib.call` was given; an argument that _lib.SIGNATURES types as
a pointer is replaced by whether it is null (addresses differ from process to process).  Two processes at the parent commit wrote
identical files, so no other argument is masked."""
import json
import numbers
import os
import sys

import pytest
import torch

from _pkg import pkg, sub
from oracle import vqa_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forward_launches.json")
IDX = [2, 0, 0, 2, 2, 0, 2]              # U = 3 images, N = 7 questions (tests/test_gpu_multi_question.py)


class _Launches:
    """Records (name, args) of every launch through _lib._HOOK, chained to the hook that was there, which is put back on exit."""

    def __init__(self):
        self.entries = []

    def __enter__(self):
        L = sub("_lib")
        prev = self._prev = L._HOOK[0]

        def hook(name, args):
            sig = L.SIGNATURES[name]
            row = [name]
            for a, t in zip(args, sig):
                if t is L.P:
                    row.append(a is None or a == 0)
                elif isinstance(a, bool) or isinstance(a, numbers.Integral):
                    row.append(int(a))
                else:
                    row.append(float(a))
            assert len(args) == len(sig) - 1, name       # (the stream is appended by _lib.call)
            self.entries.append(row)
            return prev(name, args) if prev is not None else None
        L._HOOK[0] = hook
        return self

    def __exit__(self, *exc):
        sub("_lib")._HOOK[0] = self._prev


def _engine(dtype, precision="bf16"):
    cfg = O.full_config()
    m = pkg().load_dropin().VQAModel(**cfg, compute_dtype=dtype)
    m.load_state_dict(O.init_state_dict(cfg, 11, jitter=True))
    m = m.to(DEV).eval()
    m.graph_inference = False
    if precision != "bf16":
        m.set_inference_precision(precision)
    return m, m._ensure_engine()


def _inputs(n_images, n_questions):
    images, _, _, _ = O.synthetic_batch(n_images, seed=5, image_size=224)
    _, ids, mask, _ = O.synthetic_batch(n_questions, seed=6)
    mask[:, 0] = 1
    return images.to(DEV).float().contiguous(), ids.to(DEV).long().contiguous(), mask.to(DEV).float().contiguous()


def _forward(eng, training, need_tape, indexed):
    x, ids, maskf = _inputs(3, 7) if indexed else _inputs(4, 4)
    idx = torch.tensor(IDX, device=DEV, dtype=torch.int32) if indexed else None
    with _Launches() as rec:
        eng.forward(x, ids, maskf, training=training, need_tape=need_tape, kv_index=idx)
    return rec.entries


def _encode_answer(eng, want_aux):
    x, ids, maskf = _inputs(3, 7)
    idx = torch.tensor(IDX, device=DEV, dtype=torch.int32)
    with _Launches() as rec:
        ctx = eng.encode_images(x, want_aux=want_aux)
        eng.answer(ctx, ids, maskf, idx, want_aux=want_aux)
    return rec.entries


ROUTES = {                                # name: (compute dtype, infer_precision, run(engine) -> launch list)
    "a_train_taped": ("bf16", "bf16", lambda e: _forward(e, True, True, False)),
    "b_train_taped_kv_index": ("bf16", "bf16", lambda e: _forward(e, True, True, True)),
    "c_eval": ("bf16", "bf16", lambda e: _forward(e, False, False, False)),
    "d_encode_answer": ("bf16", "bf16", lambda e: _encode_answer(e, False)),
    "e_encode_answer_aux": ("bf16", "bf16", lambda e: _encode_answer(e, True)),
    "f_eval_mxfp8": ("bf16", "mxfp8", lambda e: _forward(e, False, False, False)),
    "g_encode_answer_mxfp8": ("bf16", "mxfp8", lambda e: _encode_answer(e, False)),
    "h_eval_fp32": ("fp32", "bf16", lambda e: _forward(e, False, False, False)),
}


def _record(route):
    dtype, precision, run = ROUTES[route]
    m, eng = _engine(dtype, precision)     # a fresh model per route: step_id (dropout seeds) and the fold caches start from zero
    with torch.no_grad():
        entries = run(eng)
    torch.cuda.synchronize()
    return entries


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_route_launches_match_parent(route, golden):
    """Every launch of the route, in order, with every argument (pointers as null / non-null; nothing else is masked: two
    processes at the parent commit recorded identical lists)."""
    got, exp = _record(route), golden[route]
    assert len(exp) > 50
    for i, (g, e) in enumerate(zip(got, exp)):
        assert g == e, f"{route}: launch {i} differs: got {g}, the parent issued {e}"
    assert len(got) == len(exp), f"{route}: {len(got)} launches, the parent issued {len(exp)}"


def _write(path):
    out = {route: _record(route) for route in sorted(ROUTES)}
    with open(path, "w") as f:            # one launch per line: a changed launch shows as a changed line
        f.write("{\n")
        for k, (route, entries) in enumerate(out.items()):
            f.write(json.dumps(route) + ": [\n")
            f.write(",\n".join(json.dumps(e, separators=(",", ":")) for e in entries))
            f.write("\n]" + ("," if k + 1 < len(out) else "") + "\n")
        f.write("}\n")
    print(f"wrote {path}: " + ", ".join(f"{r} {len(e)}" for r, e in out.items()))


if __name__ == "__main__":
    if "--write" not in sys.argv:
        raise SystemExit("usage: python tests/test_gpu_forward_launches.py --write [PATH]")
    rest = [a for a in sys.argv[1:] if a != "--write"]
    _write(rest[0] if rest else GOLDEN)
