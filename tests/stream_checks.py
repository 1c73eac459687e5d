"""Stream-order checks: a harness that logs every `A.wait_stream(B)` of a step as a fork or a join, delays one
side of chosen edges with a device-side sleep, can leave one edge out, and a checker that compares two runs bit for bit.

While a `StreamHarness` is active it replaces `wait_stream` of the stream class (torch.cuda.Stream, where that method is plain
Python: `self.wait_event(stream.record_event())`); nothing in dclip_amd/ is patched.  The harness talks to the streams through a
small backend object, so the CPU tests drive it with fake streams (tests/test_stream_checks_cpu.py) and this module imports
without a GPU.

Edges.  The first time a stream appears as A the awaited B becomes its parent; an edge whose B is A's parent is a FORK, an edge
whose A is B's parent is a JOIN.  (`ROOTS` — main, the throwaway warm-up stream of GraphedStep, a capture's stream — are never a
side stream's child: a side stream seen under another root is re-parented, root -> child stays a fork, child -> root a join.)  An edge is logged with its ordinal within the
step, both names, the kind and the call site: `file:line` of the first frame inside dclip_amd/.

Schedules.  A schedule maps an edge to a list of (stream, "before" | "after") at which the harness queues a sleep:
  late(X...)   on the child X right after every fork of X ("all": every side stream) — a consumer without a join, an operand freed
               or reused while X still reads it, scratch or caches shared with a concurrent lane;
  late("main") on the PARENT right after every fork — a side stream overwriting what its parent still reads;
  head_main()  one sleep at the head of the step (`begin_step`) on the current stream — the host runs ahead of the device.
Nothing is injected while the current stream is capturing, or outside the `with`."""
from __future__ import annotations

import dataclasses
import os
import sys
from typing import Callable, Dict, Iterable, List, Optional, Tuple

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRODUCT = os.path.join(REPO, "dclip_amd") + os.sep

FLOOR_MS, CAP_MS, BUDGET_MS = 1.0, 50.0, 1000.0
SIDE = ("text", "teacher", "teacher_text", "wgrad")
ROOTS = ("main", "warmup", "capture")


# ------------------------------------------------------------------------------------------------ call sites by their text

# name -> (file under dclip_amd/, the statement, which occurrence).  The line numbers are looked up in the source as it is, so an
# edit that moves a line does not break a route assertion and an edit that removes or doubles an edge does.
_SITE_TEXT = {
    "text_fork": ("CLIP_image_distillation.py", "self._text_stream.wait_stream(main)", 0),
    "text_join": ("CLIP_image_distillation.py", "main.wait_stream(self._text_stream)", 0),
    "teacher_fork_prefetch": ("CLIP_image_distillation.py", "self._teacher_stream.wait_stream(main)", 0),
    "teacher_fork_beside": ("CLIP_image_distillation.py", "self._teacher_stream.wait_stream(main)", 1),
    "teacher_join_prefetched": ("CLIP_image_distillation.py", "main.wait_stream(self._teacher_stream)", 0),
    "teacher_join_beside": ("CLIP_image_distillation.py", "main.wait_stream(self._teacher_stream)", 1),
    "teacher_text_fork": ("patch_text_aggregation.py", "side.wait_stream(here)", 0),
    "teacher_text_join": ("patch_text_aggregation.py", "here.wait_stream(side)", 0),
    "wgrad_fork": ("engine.py", "self.side.wait_stream(self.main)", 0),
    "wgrad_join": ("engine.py", "self.main.wait_stream(self.side)", 0),
    "warmup_fork": ("graph.py", "side.wait_stream(torch.cuda.current_stream(dev))", 0),
    "warmup_join": ("graph.py", "torch.cuda.current_stream(dev).wait_stream(side)", 0),
}
_SITE_COUNT = {"CLIP_image_distillation.py": 6, "patch_text_aggregation.py": 2, "engine.py": 2, "graph.py": 2}


def find_sites(root: str = PRODUCT) -> Dict[str, str]:
    """{site name: "file:line"} of every wait_stream call of the product; raises where a statement is gone or the number of
    wait_stream calls of a file is not the listed one (a new edge needs a row in DESIGN.md §33's table and a name here)."""
    out, lines_of = {}, {}
    for name, (fname, text, nth) in _SITE_TEXT.items():
        if fname not in lines_of:
            with open(os.path.join(root, fname), encoding="utf-8") as f:
                lines_of[fname] = f.read().split("\n")
        hits = [i + 1 for i, ln in enumerate(lines_of[fname]) if ln.strip().startswith(text)]
        if len(hits) <= nth:
            raise LookupError(f"{fname}: statement {text!r} #{nth} not found")
        out[name] = f"{fname}:{hits[nth]}"
    for fname, lines in lines_of.items():
        n = sum(1 for ln in lines if ".wait_stream(" in ln and not ln.strip().startswith("#"))
        if n != _SITE_COUNT[fname]:
            raise LookupError(f"{fname}: {n} wait_stream calls, {_SITE_COUNT[fname]} listed")
    return out


# ------------------------------------------------------------------------------------------------ edges and schedules

@dataclasses.dataclass(frozen=True)
class Edge:
    step: int
    ordinal: int            # within the step
    a: str                  # the stream that waits
    b: str                  # the stream waited for
    kind: str               # "fork" | "join" | "cross"
    site: str               # file:line of the first frame inside the product
    capturing: bool = False
    dropped: bool = False

    @property
    def child(self) -> str:
        return self.a if self.kind == "fork" else self.b

    @property
    def parent(self) -> str:
        return self.b if self.kind == "fork" else self.a


@dataclasses.dataclass(frozen=True)
class Schedule:
    name: str
    at: Callable[[Edge], List[Tuple[str, str]]]      # edge -> [(stream name, "before" | "after")]
    head: bool = False                               # one sleep at the head of every step on the current stream


def no_delay() -> Schedule:
    return Schedule("none", lambda e: [])


def late(*streams: str) -> Schedule:
    names = set(SIDE) if streams == ("all",) else set(streams)
    if names == {"main"}:
        return Schedule("late(main)", lambda e: [(e.parent, "after")] if e.kind == "fork" else [])
    if "main" in names or not names:
        raise ValueError(f"late{streams!r}: main alone, or side streams")
    label = "all" if streams == ("all",) else ",".join(streams)
    return Schedule(f"late({label})", lambda e: [(e.child, "after")] if e.kind == "fork" and e.child in names else [])


def head_main() -> Schedule:
    return Schedule("head(main)", lambda e: [], head=True)


# ------------------------------------------------------------------------------------------------ backends

class TorchBackend:
    """torch.cuda streams.  Imported lazily: the module itself needs no GPU."""

    def __init__(self):
        import torch
        self.torch = torch
        self.stream_cls = torch.cuda.Stream
        self._per_ms = None

    def current(self):
        return self.torch.cuda.current_stream()

    def capturing(self) -> bool:
        return bool(self.torch.cuda.is_current_stream_capturing())

    def sleep(self, stream, cycles: int) -> None:
        with self.torch.cuda.stream(stream):
            self.torch.cuda._sleep(int(cycles))

    def cycles_per_ms(self) -> float:
        """Once per process: two events around torch.cuda._sleep(10**7) (after one untimed call: the first launch loads code)."""
        if self._per_ms is None:
            t = self.torch
            t.cuda._sleep(1000)
            t.cuda.synchronize()
            e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
            e0.record()
            t.cuda._sleep(10 ** 7)
            e1.record()
            e1.synchronize()
            self._per_ms = 10 ** 7 / max(e0.elapsed_time(e1), 1e-3)
        return self._per_ms


def runs_beside(a, b, ms: float = 2.0) -> bool:
    """Does work queued on torch stream `b` run while `a` sleeps?  False: the two share a hardware queue (a process has 4, the
    step up to 5 streams), so `b` cannot be seen running ahead of `a`.  Synchronises; a diagnostic for the controls."""
    import torch
    be = torch_backend()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(b):
        e0.record()
    be.sleep(a, max(1, int(ms * be.cycles_per_ms())))
    with torch.cuda.stream(b):
        torch.cuda._sleep(1000)
        e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) < 0.5 * ms


_TORCH_BACKEND = None


def torch_backend() -> TorchBackend:
    global _TORCH_BACKEND
    if _TORCH_BACKEND is None:
        _TORCH_BACKEND = TorchBackend()
    return _TORCH_BACKEND


def sleep_ms_for(step_ms: float, sleeps: int = 1) -> float:
    """Twice the undelayed step, floor 1 ms, cap 50 ms per sleep — and never more than the test's 1 s budget shared among the
    `sleeps` the schedule will queue (a layer-wise fork, such as the weight-gradient stream's four per layer, multiplies them)."""
    ms = min(max(2.0 * float(step_ms), FLOOR_MS), CAP_MS)
    if sleeps > 0:
        ms = min(ms, 0.95 * BUDGET_MS / sleeps)
    return max(ms, FLOOR_MS)


def module_namer(module=None, main=None, extra: Optional[Dict[str, Callable[[], object]]] = None):
    """Names a stream by the attribute it hangs from: `main` (the stream current when the harness was entered),
    module._text_stream `text`, module._teacher_stream `teacher`, module.teacher._text_side_stream `teacher_text`,
    engine._WGRAD_STREAMS[...] `wgrad`; a stream that hangs from nothing and is met at a call site in graph.py is the
    throwaway `warmup` stream (the harness calls the stream of a capture `capture`)."""
    warmups = []

    def name(stream, site: str, capturing: bool = False) -> str:
        holders = []
        if module is not None:
            holders += [("text", getattr(module, "_text_stream", None)), ("teacher", getattr(module, "_teacher_stream", None)),
                        ("teacher_text", getattr(getattr(module, "teacher", None), "_text_side_stream", None))]
        eng = sys.modules.get("dclip_amd.engine")
        holders += [("wgrad", s) for s in (getattr(eng, "_WGRAD_STREAMS", {}) or {}).values()]
        holders += [(k, fn()) for k, fn in (extra or {}).items()]
        # the object a call site passes IS the attribute, except for torch.cuda.current_stream(), which is a new object each
        # time.  Identity first: torch hands streams out of a pool of 32 per device, so a stream made later can be the same
        # queue as an older one (the long-lived weight-gradient stream, say) and compare equal to it.  For the same reason the
        # streams that hang from nothing — the warm-up's, a capture's — are recognised BEFORE any comparison by value
        for k, s_ in holders:
            if s_ is stream:
                return k
        if main is not None and stream == main:
            return "main"
        if capturing:
            return "capture"         # torch.cuda.graph captures on a stream of its own: the one stream current there
        if any(stream == w for w in warmups):
            return "warmup"
        if site.startswith("graph.py:"):
            warmups.append(stream)
            return "warmup"
        for k, s_ in holders:
            if s_ is not None and stream == s_:
                return k
        return "unknown"
    name.takes_capturing = True
    return name


# ------------------------------------------------------------------------------------------------ the harness

class StreamHarness:
    def __init__(self, schedule: Optional[Schedule] = None, namer=None, drop: Iterable[int] = (), drop_steps=None,
                 sleep_ms: float = 0.0, backend=None, product_root: str = PRODUCT, drop_sites: Iterable[str] = ()):
        """`drop`: ordinals (within the step) of edges that are NOT executed — or `drop_sites`: their call sites — in the steps
        of `drop_steps` (None: every step); for the controls only.  `sleep_ms`: length of each injected sleep."""
        self.schedule = schedule or no_delay()
        self.backend = backend if backend is not None else torch_backend()
        self.namer = namer
        self.drop = frozenset(int(k) for k in drop)
        self.drop_sites = frozenset(drop_sites)
        self.drop_steps = None if drop_steps is None else frozenset(drop_steps)
        self.sleep_ms = float(sleep_ms)
        self.root = product_root
        self.edges: List[Edge] = []
        self.sleeps: List[Tuple[int, int, str, str]] = []         # (step, ordinal or -1 for the head, stream name, moment)
        self.injected_ms = 0.0
        self.step, self._ordinal = 0, 0
        self._parent: Dict[str, str] = {}
        self._active = False
        self._orig = None
        self._streams: Dict[str, object] = {}

    # ---- context
    def __enter__(self):
        cls = self.backend.stream_cls
        self._orig = cls.wait_stream
        harness, orig = self, self._orig

        def wait_stream(a, b):
            if not harness._active:
                return orig(a, b)
            return harness._edge(a, b)

        cls.wait_stream = wait_stream
        if self.namer is None:
            self.namer = module_namer(main=self.backend.current())
        self._active = True
        return self

    def __exit__(self, *exc):
        self._active = False
        self.backend.stream_cls.wait_stream = self._orig
        return False

    # ---- steps
    def begin_step(self, head: bool = True) -> None:
        """A new step: ordinals restart; `head` schedules queue their one sleep on the current stream now (`head=False`: the
        caller places it itself, with head())."""
        self.step += 1
        self._ordinal = 0
        if head:
            self.head()

    def head(self) -> None:
        if self._active and self.schedule.head and not self.backend.capturing():
            cur = self.backend.current()
            self._sleep(cur, self.namer(cur, ""), -1, "head")

    # ---- internals
    def _site(self) -> str:
        f = sys._getframe(2)
        while f is not None:
            fn = os.path.abspath(f.f_code.co_filename)
            if fn.startswith(self.root):
                rel = os.path.relpath(fn, self.root) if os.path.isdir(self.root) else os.path.basename(fn)
                return f"{rel}:{f.f_lineno}"
            f = f.f_back
        return "?:0"

    def _sleep(self, stream, name: str, ordinal: int, moment: str) -> None:
        if self.sleep_ms <= 0.0:
            return
        self.backend.sleep(stream, max(1, int(self.sleep_ms * self.backend.cycles_per_ms())))
        self.sleeps.append((self.step, ordinal, name, moment))
        self.injected_ms += self.sleep_ms

    def _kind(self, a: str, b: str) -> str:
        """Roots (`ROOTS`: main, the warm-up stream, a capture's stream) are never children of a side stream: a side stream that
        waits for a root is forked from it (and re-parented: warm-up, then capture, then main), a root that waits for a side
        stream joins it.  Otherwise the first B a stream waits for is its parent."""
        par = self._parent
        if par.get(a) == b:
            return "fork"
        if par.get(b) == a:
            return "join"
        ra, rb = a in ROOTS, b in ROOTS
        if rb and not ra:
            par[a] = b
            return "fork"
        if ra and not rb:
            par[b] = a
            return "join"
        if a not in par and a != "main":
            par[a] = b                                   # first time as A: B is its parent
            return "fork"
        return "cross"

    def _edge(self, a, b):
        site = self._site()
        capturing = self.backend.capturing()
        if getattr(self.namer, "takes_capturing", False):
            na, nb = self.namer(a, site, capturing), self.namer(b, site, capturing)
        else:
            na, nb = self.namer(a, site), self.namer(b, site)
        if capturing:            # torch.cuda.graph captures on a stream of its own, which hangs from nothing
            na, nb = ("capture" if n == "unknown" else n for n in (na, nb))
        self._streams[na], self._streams[nb] = a, b
        k = self._ordinal
        self._ordinal += 1
        dropped = (not capturing) and (k in self.drop or site in self.drop_sites) \
            and (self.drop_steps is None or self.step in self.drop_steps)
        e = Edge(self.step, k, na, nb, self._kind(na, nb), site, capturing, dropped)
        self.edges.append(e)
        where = [] if capturing else self.schedule.at(e)
        for name, moment in where:
            if moment == "before":
                self._sleep(self._streams[name], name, k, moment)
        if not dropped:
            self._orig(a, b)
        for name, moment in where:
            if moment == "after":
                self._sleep(self._streams[name], name, k, moment)

    # ---- reading the log
    def pairs(self, step: Optional[int] = None, capturing: Optional[bool] = None) -> List[Tuple[str, str]]:
        return [(e.site, e.kind) for e in self.edges if (step is None or e.step == step)
                and (capturing is None or e.capturing == capturing)]

    def streams_seen(self) -> set:
        return {n for e in self.edges for n in (e.a, e.b)}

    def describe(self) -> str:
        return "\n".join(f"  step {e.step} #{e.ordinal} {e.a} waits {e.b}: {e.kind} at {e.site}"
                         f"{' (capturing)' if e.capturing else ''}{' DROPPED' if e.dropped else ''}" for e in self.edges)


def count_sleeps(edges: Iterable[Edge], schedule: Schedule, steps: int = 0) -> int:
    """How many sleeps `schedule` queues over a logged run (`steps`: the heads of a head schedule)."""
    return sum(len(schedule.at(e)) for e in edges if not e.capturing) + (steps if schedule.head else 0)


# ------------------------------------------------------------------------------------------------ the checker

class BitsDiffer(AssertionError):
    pass


_INT_OF = {1: "int8", 2: "int16", 4: "int32", 8: "int64"}


def _words(t):
    import torch
    t = t.detach().contiguous()
    if t.dtype == torch.bool:
        return t.to(torch.int8)
    return t.view(getattr(torch, _INT_OF[t.element_size()]))


def first_difference(got, want):
    """None, or (flat index, got value, want value) of the first element whose WORD differs (NaNs compare as their bits)."""
    import torch
    g, w = _words(got).reshape(-1), _words(want.to(got.device)).reshape(-1)
    ne = g != w
    if not bool(ne.any()):
        return None
    i = int(torch.nonzero(ne)[0])
    return i, got.detach().reshape(-1)[i].item(), want.detach().reshape(-1)[i].item()


def assert_same_bits(got: Dict[str, object], want: Dict[str, object], exceptions: Optional[Dict[str, object]] = None,
                     what: str = "") -> None:
    """`got` and `want`: {name: tensor} — the loss, every last_losses entry, every parameter gradient and (multi-step cases)
    every parameter, per step.  Same names, shapes and types, and every value the same integer word.  `exceptions`: {name:
    bound} — the one admitted family is the `tok` gradient of a TRAINABLE text tower (float atomics in no fixed order), which
    passes under schedule_checks.embed_atomic_bound = c * 2^-24 * sum|dx| per element instead.  Reports the first tensor that
    differs, in `want`'s order, and its first element."""
    exceptions = exceptions or {}
    if list(got.keys()) != list(want.keys()):
        only_g, only_w = [k for k in got if k not in want], [k for k in want if k not in got]
        raise BitsDiffer(f"{what}: names differ (only got: {only_g[:4]}, only want: {only_w[:4]})")
    for name, w in want.items():
        g = got[name]
        if (g is None) != (w is None):
            raise BitsDiffer(f"{what}: {name}: one side is None")
        if w is None:
            continue
        if tuple(g.shape) != tuple(w.shape) or g.dtype != w.dtype:
            raise BitsDiffer(f"{what}: {name}: {tuple(g.shape)}/{g.dtype} against {tuple(w.shape)}/{w.dtype}")
        if name in exceptions:
            bound = exceptions[name]
            err = (g.double() - w.to(g.device).double()).abs()
            over = ~(err <= (bound.to(g.device) if hasattr(bound, "to") else bound))          # a NaN is over any bound
            if bool(over.any()):
                raise BitsDiffer(f"{what}: {name}: outside its bound at {int(over.reshape(-1).nonzero()[0])}")
            continue
        d = first_difference(g, w)
        if d is not None:
            raise BitsDiffer(f"{what}: first differing tensor {name}, element {d[0]} of {g.numel()}: got {d[1]!r}, want {d[2]!r}")


def differing(got: Dict[str, object], want: Dict[str, object]) -> List[str]:
    """Names whose words differ (for the controls, which expect a difference)."""
    return [n for n, w in want.items() if w is not None and n in got and got[n] is not None
            and first_difference(got[n], w) is not None]
