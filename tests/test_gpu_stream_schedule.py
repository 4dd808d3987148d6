"""Stream schedules: a step computes the same bits whichever of its streams runs late.

The engine issues its launches on up to three streams (main; `engine.side`: the text encoder and the hoisted cross-attention K | V;
`engine.side2`: weight gradients, operand packing, parameter-gradient folds), ordered by hand-placed events and with hand-managed
tensor lifetimes ("Cross-stream hand-offs").  A missing wait or a tensor freed under a side-stream reader faults nothing
and, at natural timing, usually changes nothing.  Here every route runs under five schedules -- serial (`two_streams = False`),
overlapped, and overlapped with main, side or side2 made slow by a spin in front of each of its launches (tests/_streamskew.py) --
three consecutive steps each, on a fresh model and trainer from one state dict, and every result is compared bit for bit.

The delay D per launch is sized from the route itself: the serial run times every launch between two events of its stream (the
same hook; _longest_launch takes the last two steps) and D = max(100 us, 10 x the longest launch), so that a consumer on an
undelayed stream certainly reaches its launch while its producer still sits behind the spin.  The spin is calibrated once per
process (_streamskew.calibrate).

Measured on an MI355X (`pytest -s` prints these lines again): 2393 spin cycles per microsecond -- not the 1500 that the engine's
"1.5 M cycles ~ 1 ms" assumes.  Per route: launches through the hook in one step, the longest of them, the chosen D, and the
launches of three overlapped steps on main / side / side2.

    route              fp32: launches  longest launch          D        main side side2 | bf16: launches  longest launch             D       main side side2
    step                     336       vqa_dgrad_s2 151 us     1506 us   678  289   89  |       288       vqa_conv8p 93 us           930 us   535  289   89
    step_grouped             337       vqa_dgrad_s2 150 us     1501 us   681  289   89  |       289       vqa_conv8p 94 us           936 us   538  289   89
    step_features            209       vqa_igemm 120 us        1204 us   334  289   32  |       210       vqa_fold_bn_batch 48 us    478 us   338  289   32
    step_frozen_cnn          209       vqa_igemm 121 us        1211 us   334  289   32  |       209       vqa_fold_bn_batch 53 us    526 us   335  289   32
    autograd                 335       vqa_dgrad_s2 150 us     1504 us   675  289   89  |       288       vqa_conv8p 94 us           939 us   534  289   89
    autograd_aux             341       vqa_dgrad_s2 150 us     1503 us   693  289   89  |       298       vqa_conv8p 92 us           916 us   564  289   89
    eval                     175       vqa_igemm 121 us        1209 us   321  204    0  |       177       vqa_igemm 45 us            445 us   327  204    0
    encode_answer             87       vqa_igemm 120 us        1203 us   261    0    0  |        88       vqa_igemm 45 us            446 us   264    0    0
    explain                  155       vqa_igemm 119 us        1194 us   472    6    0  |       156       vqa_conv8p 80 us           796 us   475    6    0
    step_full (default widths, B = 5)                                                   |       261       vqa_adamw 104 us          1038 us   485  241  107
    step + reducer                                                                      |       288       vqa_conv8p 92 us           916 us   535  289   89

The small configuration's launches are short and latency-bound, so a span is mostly what a launch costs at all; D is the same order
for every route, and a skewed step takes 0.1 - 1 s.  Serial and overlapped turned out bit-equal for every tensor of every route:
`two_streams = False` changes where launches run, never their arithmetic, so no tensor needs a tolerance.  No schedule differed
from another: no hazard was found.  The reducer case (its own process, a one-rank gloo group) puts a spin of max(D, 5 ms) on the
communication stream ahead of each message.  The whole module takes about 35 s, no test more than 4.3 s."""
import os
import socket
import time

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

from _pkg import pkg, sub
from _streamskew import calibrate, skew
from oracle import vqa_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
SMALL = dict(vocab_size=100, num_answers=10, embed_dim=32)
CFG_SMALL = O.full_config(dropout=0.1, answer_dropout=0.1, **SMALL)
CFG_FULL = O.full_config(dropout=0.1, answer_dropout=0.1)
GROUP_INDEX = [0, 1, 1, 0, 1, 0, 0]          # U = 3 images, N = 7 questions
STEPS = 3
D_FLOOR_US = 100.0
COMM_DELAY_US = 5000.0
AUX_KEYS = ("image_features", "text_features", "text_pooled", "fused", "image_projected", "attended_pooled")
_CACHE = {}

# Streams each route issues launches on when overlapped ("Cross-stream hand-offs", lists the edges between them).  A
# schedule that slows a stream the route never uses would equal the unskewed one launch for launch and is not run.
#   eval forward: no backward, so nothing is packed or reduced on side2
#   encode_images + answer: the two halves of the eval forward, each on the caller's stream alone
#   explain: the backward stops at the image features and computes no parameter gradient; only the hoisted K | V path (forward
#            and backward) leaves main
ROUTE_STREAMS = {
    "step": ("main", "side", "side2"),
    "step_grouped": ("main", "side", "side2"),
    "step_features": ("main", "side", "side2"),
    "step_frozen_cnn": ("main", "side", "side2"),
    "autograd": ("main", "side", "side2"),
    "autograd_aux": ("main", "side", "side2"),
    "eval": ("main", "side"),
    "encode_answer": ("main",),
    "explain": ("main", "side"),
    "step_full": ("main", "side", "side2"),
}


def _small(name):
    return name != "step_full"


def _sd(name):
    key = ("sd", _small(name))
    if key not in _CACHE:
        _CACHE[key] = O.init_state_dict(CFG_SMALL if _small(name) else CFG_FULL, 41, jitter=True)
    return _CACHE[key]


def _batch(name, k):
    key = ("batch", _small(name), k)
    if key not in _CACHE:
        if _small(name):
            b = O.synthetic_batch(7, seed=300 + k, image_size=64, seq_len=10, vocab=100, num_answers=10)
        else:
            b = O.synthetic_batch(5, seed=300 + k)
        _CACHE[key] = [t.to(DEV) for t in b]
    return _CACHE[key]


def _bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def _snap(pairs):
    return [(n, t.detach().clone()) for n, t in pairs]


# ------------------------------------------------------------------------------------------------------------------- the routes
class _Route:
    """A fresh model (and trainer) from the shared state dict; call(k) runs the k-th step and returns [(name, tensor)] in the order
    the step produces them, cloned on the main stream (no host synchronisation between steps: the host stays ahead of the device)."""

    def __init__(self, name, dtype, **trainer_kw):
        self.name, self.dtype = name, dtype
        cfg = CFG_SMALL if _small(name) else CFG_FULL
        m = pkg().load_dropin().VQAModel(**cfg, compute_dtype=dtype)
        m.load_state_dict(_sd(name))
        self.m = m.to(DEV).train()
        self.m.graph_inference = False                         # eager everywhere: a replayed graph cannot be skewed from the hook
        self.tr = None
        if name in ("step_features", "step_frozen_cnn"):
            self.m.image_encoder.requires_grad_(False)
            self.m.image_encoder.eval()
        if name in ("eval", "encode_answer", "explain"):
            self.m.eval()
        if name.startswith("step"):
            self.tr = pkg().trainer.HipTrainer(self.m, lr=1e-3, **trainer_kw)
        self.engine = self.m._ensure_engine()

    def _buffers(self):
        return [("buffer " + n, b) for n, b in sorted(self.m.named_buffers())]

    def call(self, k):
        images, ids, mask, answers = _batch(self.name, k)
        m, name = self.m, self.name
        if name.startswith("step"):
            idx = None
            if name == "step_grouped":
                images, idx = images[:3].contiguous(), torch.tensor(GROUP_INDEX)
            if name == "step_features":
                m.eval()
                with torch.no_grad():
                    images = m.encode_features(images)
                m.train()
                m.image_encoder.eval()
            loss, logits = self.tr.step(images, ids, mask, answers, image_index=idx)
            out = self._buffers() + [("logits", logits), ("loss", loss), ("gradient buffer", self.tr.G), ("parameters", m._flat),
                                     ("first moment", self.tr.m), ("second moment", self.tr.v)]
            copy = self.engine.adamw_copy_target()
            if self.dtype == "bf16":
                assert copy is not None
                out.append(("bf16 parameter copy", copy))
            return _snap(out)
        if name.startswith("autograd"):
            for p in m.parameters():
                p.grad = None
            x = images.clone().requires_grad_(True)
            logits, aux = m(x, ids, mask, return_aux=name == "autograd_aux")
            loss = F.cross_entropy(logits, answers)
            if aux is not None:
                loss = loss + sum(aux[key].float().square().mean() for key in AUX_KEYS) \
                    + sum(w.float().square().mean() for w in aux["cross_attention_weights"])
            loss.backward()
            grads = [("grad " + n, p.grad) for n, p in m.named_parameters()]
            assert all(g is not None for _, g in grads) and x.grad is not None
            return _snap(self._buffers() + [("logits", logits), ("loss", loss)] + grads + [("image gradient", x.grad)])
        with torch.no_grad():
            if name == "eval":
                logits, _ = m(images, ids, mask)
                logits2, aux = m(images, ids, mask, return_aux=True)
                out = [("logits", logits), ("logits (aux call)", logits2)] + [("aux " + key, aux[key]) for key in AUX_KEYS]
                out += [(f"aux cross_attention_weights[{i}]", w) for i, w in enumerate(aux["cross_attention_weights"])]
                return _snap(out)
            if name == "encode_answer":
                ctx = m.encode_images(images[:3].contiguous())
                logits, _ = m.answer(ctx, ids, mask, image_index=torch.tensor(GROUP_INDEX))
                return _snap([("context K|V", ctx._eng["kv"]), ("logits", logits)])
            e = m.explain(images, ids, mask)
            return _snap([("logits", e.logits), ("answers", e.answers), ("gradcam", e.gradcam), ("attention", e.attention)])


def _run(name, dtype, schedule, delay_us=0.0, steps=STEPS, reducer=False):
    """One schedule of one route on a fresh model; returns (records per step, the harness, {stream name: stream}).
    reducer: the trainer runs its bucket reducer (force_reducer=True; the caller has made the process group), and the schedule
    "comm" puts the spin on the reducer's communication stream ahead of every message it issues (collectives do not pass the
    launch hook); the harness then carries their number as `comm_delayed`."""
    torch.cuda.synchronize()
    r = _Route(name, dtype, **(dict(force_reducer=True) if reducer else {}))
    eng = r.engine
    assert eng.side is not None and eng.side2 is not None and eng.two_streams
    streams = {"main": torch.cuda.current_stream(), "side": eng.side, "side2": eng.side2}
    if schedule == "serial":
        eng.two_streams = False
    slow = streams.get(schedule)
    issued = [0]
    if reducer:
        red = r.tr.reducer
        assert red.active and red.comm_stream is not None
        if schedule == "comm":
            cycles, issue = round(max(delay_us, COMM_DELAY_US) * calibrate()), red._issue      # (a handful of messages per step)

            def slow_issue(tensor, events=()):
                with torch.cuda.stream(red.comm_stream):
                    torch.cuda._sleep(cycles)
                issued[0] += 1
                return issue(tensor, events)
            red._issue = slow_issue
    starts = []
    with skew(slow=() if slow is None else slow, delay_us=delay_us if slow is not None else 0.0, timed=schedule == "serial") as s:
        recs = []
        for k in range(steps):
            starts.append(s.timed_launches)
            recs.append(r.call(k))
    torch.cuda.synchronize()
    s.step_starts, s.comm_delayed = starts + [s.timed_launches], issued[0]
    return recs, s, streams


def _longest_launch(s):
    """(name, microseconds) of the longest launch of a step of the timed serial run.  A span also holds whatever kept the host
    between its two event records, so where the last two steps issued the same launches each launch counts with the shorter of
    its two spans; otherwise the last step's spans count as they are."""
    b = s.step_starts
    last = s.durations_us(start=b[-2])
    prev = s.durations_us(start=b[-3])[: b[-2] - b[-3]] if len(b) > 2 else []
    if [n for n, _ in last] == [n for n, _ in prev]:
        last = [(n, min(t, u)) for (n, t), (_, u) in zip(last, prev)]
    return len(last), max(last, key=lambda e: e[1])


def _first_difference(a, b):
    """(step, tensor name) of the first tensor that differs, in the order the step produces them; None when all are equal."""
    assert len(a) == len(b)
    for k, (ra, rb) in enumerate(zip(a, b)):
        assert [n for n, _ in ra] == [n for n, _ in rb]
        for (n, x), (_, y) in zip(ra, rb):
            if x.dtype != y.dtype or x.shape != y.shape or not torch.equal(_bits(x), _bits(y)):
                return k, n
    return None


def _check_counters(name, schedule, s, streams):
    used = ROUTE_STREAMS[name]
    on = {n: s.launches_on(st) for n, st in streams.items()}
    assert sum(on.values()) == sum(s.launches.values()), "launches on a stream that is none of main, side, side2"
    if schedule == "serial":
        assert on["main"] > 0 and on["side"] == 0 and on["side2"] == 0, on
        assert not s.delayed
        return
    for n in streams:                                          # the route's table above, both ways
        assert (on[n] > 0) == (n in used), (name, schedule, on)
    if schedule == "overlapped":
        assert not s.delayed
    elif schedule == "comm":                                   # the reducer's messages were delayed, and no launch
        assert not s.delayed and s.comm_delayed > 0
    else:                                                      # every launch of the slowed stream was delayed, and no other
        assert s.delayed_on(streams[schedule]) == on[schedule] > 0
        assert sum(s.delayed.values()) == on[schedule]


def _five_schedules(name, dtype, steps=STEPS, reducer=False):
    """Serial, overlapped, and one skewed schedule per stream of the route's row in ROUTE_STREAMS (reducer: and one with the
    communication stream slow); every record of every step equal to the unskewed overlapped one's, bit for bit.  Returns the line
    it prints."""
    serial, s_serial, streams = _run(name, dtype, "serial", steps=steps, reducer=reducer)
    _check_counters(name, "serial", s_serial, streams)
    per_step, longest = _longest_launch(s_serial)
    delay = max(D_FLOOR_US, 10.0 * longest[1])
    base, s_base, streams = _run(name, dtype, "overlapped", steps=steps, reducer=reducer)
    _check_counters(name, "overlapped", s_base, streams)
    line = (f"[{name}-{dtype}{' + reducer' if reducer else ''}] {per_step} launches in a step, longest {longest[0]} {longest[1]:.1f} us, "
            f"D = {delay:.0f} us, {calibrate():.0f} spin cycles per us; launches per {steps} steps: "
            + ", ".join(f"{n} {s_base.launches_on(st)}" for n, st in streams.items()))
    print("\n" + line)
    assert all(bool(torch.isfinite(t).all()) for n, t in base[-1] if n in ("loss", "logits"))
    d = _first_difference(base, serial)
    assert d is None, ("serial differs from overlapped at (step, tensor)", d)
    for schedule in ROUTE_STREAMS[name] + (("comm",) if reducer else ()):
        got, s, streams = _run(name, dtype, schedule, delay_us=delay, steps=steps, reducer=reducer)
        _check_counters(name, schedule, s, streams)
        d = _first_difference(base, got)
        assert d is None, (f"{schedule} slow differs from unskewed at (step, tensor)", d)
    return line


# ------------------------------------------------------------------------------------------- a: the harness sees a missing wait
@pytest.mark.parametrize("wait", [True, False])
def test_skew_exposes_a_missing_event_wait_between_two_streams(wait):
    """Test-owned buffers only.  The producer (vqa_add on main) writes over a sentinel; the consumer (vqa_add on a second stream)
    copies what it finds.  Main is slow: with the event wait the consumer sees the produced values, without it the sentinel."""
    L, E = sub("_lib"), sub("engine")
    n = 4096
    main = torch.cuda.current_stream()
    (second,) = E.pick_concurrent_streams(torch.device(DEV), 1)
    assert E._streams_overlap(main, second, cycles=round(5000 * calibrate()))
    src = torch.arange(n, device=DEV, dtype=torch.float32)
    zero = torch.zeros(n, device=DEV)
    buf = torch.full((n,), -7.0, device=DEV)
    out = torch.full((n,), -1.0, device=DEV)
    torch.cuda.synchronize()
    with skew(slow=main, delay_us=5000.0) as s:
        L.call("vqa_add", 0, L.ptr(src), L.ptr(zero), L.ptr(buf), n)            # main, behind a 5 ms spin
        ev = torch.cuda.Event(); ev.record(main)
        if wait:
            second.wait_event(ev)
        with torch.cuda.stream(second):
            L.call("vqa_add", 0, L.ptr(buf), L.ptr(zero), L.ptr(out), n)
    torch.cuda.synchronize()
    assert s.launches_on(main) == 1 and s.delayed_on(main) == 1 and s.launches_on(second) == 1 and s.delayed_on(second) == 0
    assert torch.equal(buf, src)
    assert torch.equal(out, src if wait else torch.full_like(src, -7.0))


# ---------------------------------------------------------------------------------------------------- b: the streams do overlap
def test_engine_streams_overlap_pairwise():
    """Without this the comparisons below would pass vacuously on a machine where the streams share a hardware queue."""
    E = sub("engine")
    eng = _Route("eval", "fp32").engine
    assert eng.side is not None and eng.side2 is not None
    main = torch.cuda.current_stream()
    spin = round(5000 * calibrate())                           # 5 ms on the first stream: the host has ample time to query it
    for a, b in ((main, eng.side), (main, eng.side2), (eng.side, eng.side2), (eng.side, main), (eng.side2, main), (eng.side2, eng.side)):
        torch.cuda.synchronize()
        assert E._streams_overlap(a, b, cycles=spin), \
            "two of main, side and side2 share a hardware queue: the skewed schedules test nothing here"


# ----------------------------------------------------------------------------------------------- c: five schedules, bit for bit
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", [n for n in ROUTE_STREAMS if n != "step_full"])
def test_five_schedules_give_the_same_bits(name, dtype):
    _five_schedules(name, dtype)


def test_five_schedules_give_the_same_bits_at_default_widths():
    """embed 256, 49 image tokens, 224 x 224, B = 5, bf16: the smallest shape at which the dedicated kernels and the engine's real
    side2 plan run (conv8p, c64p, the fused stem weight gradient, the deferred last-block weight gradients, pack_off_main)."""
    _five_schedules("step_full", "bf16")


# ------------------------------------------------------------------------------------- d: the reducer's communication stream
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _reducer_worker(port, q):
    """A process of its own, so that no other test of this session sees a process group: one rank over gloo (as
    tests/test_gpu_dp.py makes its group), HipTrainer(force_reducer=True) as bench.py --force-reducer builds it."""
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=0, world_size=1)
        torch.cuda.set_device(0)
        line = _five_schedules("step", "bf16", reducer=True)   # (bf16 alone: the process start is most of this test's time)
        dist.destroy_process_group()
        q.put(("ok", line))
    except BaseException as e:                                 # the parent reports it
        q.put(("failed", f"{type(e).__name__}: {e}"))
        raise


def test_six_schedules_give_the_same_bits_with_the_bucket_reducer():
    """The plain step with the gradient buckets all-reduced on the reducer's communication stream, in a world of one rank: the
    five schedules and one with the communication stream slow."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_reducer_worker, args=(_free_port(), q))
    p.start()
    try:
        deadline = time.monotonic() + 240
        while q.empty() and p.is_alive() and time.monotonic() < deadline:      # (returns as soon as the child has answered or died)
            p.join(timeout=0.05)
        status, what = q.get(timeout=5) if (not q.empty() or not p.is_alive()) else ("failed", "no answer within 240 s")
    finally:
        p.join(timeout=30)
        if p.is_alive():
            p.kill()
    assert status == "ok", what
    assert p.exitcode == 0 and what.startswith("[step-bf16 + reducer]")
