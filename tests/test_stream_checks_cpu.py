"""The stream-order harness of tests/stream_checks.py on fake streams: per-stream FIFO queues that a small
machine executes in the order of a simulated clock, so a sleep queued on one stream really moves that stream's work behind the
others'.  Shown here: edges are logged, named and classified (the nested teacher -> teacher_text fork included), drop(k) leaves
out exactly one edge, every schedule queues its sleep where its definition says, nothing is injected while "capturing", and
three planted ordering faults of a toy two-queue program are caught by assert_same_bits under the schedule named for each —
and missed without a delay, which is kept as a test: it is why the GPU cases need the schedules at all."""
import os

import pytest
import torch

from tests import stream_checks as sc

HERE = os.path.abspath(__file__)


# ------------------------------------------------------------------------------------------------ fake streams

class Event:
    def __init__(self):
        self.time = None


class FakeStream:
    def __init__(self, machine, name):
        self.machine, self.name, self.q, self.t = machine, name, [], 0.0
        machine.streams.append(self)

    def record_event(self):
        ev = Event()
        self.q.append(("record", ev))
        return ev

    def wait_event(self, ev):
        self.q.append(("wait", ev))

    def wait_stream(self, other):                  # torch.cuda.Stream.wait_stream, word for word
        self.wait_event(other.record_event())

    def run(self, fn, dur=1.0):
        self.q.append(("run", fn, dur))


class Machine:
    """Queues first (the host runs ahead), then `drain()`: always the runnable head with the smallest clock; a kernel reads and
    writes `mem` at its start."""

    def __init__(self, names=("main", "side")):
        self.streams, self.mem, self.capturing_now, self.trace = [], {}, False, []
        for n in names:
            setattr(self, n, FakeStream(self, n))
        self.now = self.streams[0]

    # the harness's backend
    stream_cls = FakeStream

    def current(self):
        return self.now

    def capturing(self):
        return self.capturing_now

    def sleep(self, stream, cycles):
        stream.q.append(("sleep", cycles))

    def cycles_per_ms(self):
        return 1.0

    def drain(self):
        while any(s.q for s in self.streams):
            ready = []
            for i, s in enumerate(self.streams):
                if not s.q:
                    continue
                op = s.q[0]
                if op[0] == "wait":
                    if op[1].time is None:
                        continue
                    ready.append((max(s.t, op[1].time), i))
                else:
                    ready.append((s.t, i))
            assert ready, "deadlock: a wait on an event that is never recorded"
            start, i = min(ready)
            s = self.streams[i]
            op = s.q.pop(0)
            s.t = start
            if op[0] == "record":
                op[1].time = s.t
            elif op[0] == "sleep":
                self.trace.append((s.name, "sleep", s.t))
                s.t += op[1]
            elif op[0] == "run":
                self.trace.append((s.name, getattr(op[1], "__name__", "kernel"), s.t))
                op[1]()
                s.t += op[2]


def harness(m, schedule=None, **kw):
    return sc.StreamHarness(schedule, namer=lambda s, site: s.name, backend=m, product_root=HERE, **kw)


# ------------------------------------------------------------------------------------------------ the toy two-queue program

def toy(m, h, fault=None, steps=2):
    """Per step: main makes a = x + 1; fork; the side lane makes s = 2a through its scratch while main makes b = a + 10 through
    its own scratch, held across a long kernel; join; out = s + b.  Without a delay the side lane is done long before main's
    scratch is written, so each of the three faults is invisible at the natural timing."""
    main, side, mem = m.main, m.side, m.mem
    mem.update(a=0.0, s=0.0, b=0.0, scratch0=0.0, scratch1=0.0)
    outs = {}
    lane = "scratch0" if fault == "shared_scratch" else "scratch1"
    for k in range(steps):
        h.begin_step()
        x = float(k + 1)
        main.run(lambda x=x: mem.__setitem__("a", x + 1.0), 1)
        if fault != "missing_fork":
            side.wait_stream(main)
        side.run(lambda: None, 2)                                             # unrelated work of the lane
        side.run(lambda: mem.__setitem__(lane, 2.0 * mem["a"]), 1)
        side.run(lambda: mem.__setitem__("s", mem[lane]), 1)
        main.run(lambda: None, 4)
        main.run(lambda: mem.__setitem__("scratch0", mem["a"] + 10.0), 1)
        main.run(lambda: None, 20)
        main.run(lambda: mem.__setitem__("b", mem["scratch0"]), 1)
        if fault != "missing_join":
            main.wait_stream(side)
        main.run(lambda k=k: outs.__setitem__(f"step{k}.out", torch.tensor([mem["s"] + mem["b"]])), 1)
    m.drain()
    return outs


def run_toy(fault=None, schedule=None, sleep_ms=0.0, steps=2, **kw):
    m = Machine()
    with harness(m, schedule, sleep_ms=sleep_ms, **kw) as h:
        outs = toy(m, h, fault, steps)
    return outs, h, m


WANT = {"step0.out": torch.tensor([2.0 * 2.0 + 12.0]), "step1.out": torch.tensor([2.0 * 3.0 + 13.0])}
WANT1 = {"step0.out": WANT["step0.out"]}         # the planted faults run ONE step: nothing here models the host's launch order,
#                                                  which is all that holds an unforked lane's second step behind the first

# fault -> (the schedule named for it, the sleep).  The toy's undelayed step takes 28 ticks; twice that for the two faults that a
# lane running late (or a parent running late) shows.  The shared scratch needs the side lane INSIDE main's window (ticks 5..26 of
# the step): a sleep longer than main's way to the join serialises the lanes and hides it (limits).
def _late_side():
    return sc.late("side")


PLANTED = {
    "missing_join": (_late_side(), 56.0),
    "missing_fork": (sc.head_main(), 56.0),
    "shared_scratch": (_late_side(), 10.0),
}


def test_the_toy_is_right_under_every_schedule():
    base, h, m = run_toy()
    sc.assert_same_bits(base, WANT, what="toy, no delay")
    assert max(s.t for s in m.streams) == 2 * 28.0                       # the undelayed step: 28 ticks
    for sched, ms in ((_late_side(), 56.0), (_late_side(), 10.0), (sc.late("main"), 56.0), (sc.head_main(), 56.0)):
        got, h, _ = run_toy(None, sched, ms)
        sc.assert_same_bits(got, WANT, what=f"toy, {sched.name}")
        assert h.injected_ms == 2 * ms                                   # one fork, or one head, per step


@pytest.mark.parametrize("fault", sorted(PLANTED))
def test_a_planted_fault_is_caught_under_its_schedule(fault):
    sched, ms = PLANTED[fault]
    got, h, _ = run_toy(fault, sched, ms, steps=1)
    with pytest.raises(sc.BitsDiffer, match="first differing tensor step0.out, element 0 of 1"):
        sc.assert_same_bits(got, WANT1, what=fault)
    assert sc.differing(got, WANT1) == ["step0.out"] and h.injected_ms == ms


@pytest.mark.parametrize("fault", sorted(PLANTED))
def test_a_planted_fault_is_missed_without_a_delay(fault):
    """The natural timing hides all three — what every other test of the suite runs at."""
    got, h, _ = run_toy(fault, steps=1)
    sc.assert_same_bits(got, WANT1, what=fault)
    assert h.injected_ms == 0.0 and not h.sleeps


def test_a_sleep_past_the_join_hides_the_shared_scratch():
    """The limit of late(X): with a sleep longer than main's way to the join the lanes run one after the other."""
    got, _, _ = run_toy("shared_scratch", _late_side(), 56.0, steps=1)
    sc.assert_same_bits(got, WANT1)


# ------------------------------------------------------------------------------------------------ log, names, kinds

def nested(m, h, steps=1, prefetch=False):
    """The meta-teacher step's shape: main forks teacher, teacher forks teacher_text and joins it, main forks text, main joins
    teacher and text.  `prefetch`: the teacher's fork of step n is joined in step n + 1."""
    for _ in range(steps):
        h.begin_step()
        m.teacher.wait_stream(m.main)
        m.now = m.teacher
        m.teacher_text.wait_stream(m.teacher)
        m.teacher.wait_stream(m.teacher_text)
        m.now = m.main
        if not prefetch:
            m.main.wait_stream(m.teacher)
        m.text.wait_stream(m.main)
        m.main.wait_stream(m.text)
        if prefetch:
            h.begin_step()
            m.main.wait_stream(m.teacher)
    m.drain()


NAMES = ("main", "teacher", "teacher_text", "text")


def test_edges_are_logged_named_and_classified():
    m = Machine(NAMES)
    with harness(m) as h:
        nested(m, h, steps=2)
    per_step = [("teacher", "main", "fork"), ("teacher_text", "teacher", "fork"), ("teacher", "teacher_text", "join"),
                ("main", "teacher", "join"), ("text", "main", "fork"), ("main", "text", "join")]
    assert [(e.step, e.ordinal, e.a, e.b, e.kind) for e in h.edges] == \
        [(s, k, *row) for s in (1, 2) for k, row in enumerate(per_step)]
    assert h._parent == {"teacher": "main", "teacher_text": "teacher", "text": "main"}
    assert h.streams_seen() == set(NAMES)
    # the call site: file:line of the first frame inside the "product" (here: this file, the lines of nested())
    import inspect
    first = inspect.getsourcelines(nested)[1]
    base = os.path.basename(HERE)
    assert {e.site.split(":")[0] for e in h.edges} == {base}
    lines = [int(e.site.split(":")[1]) for e in h.edges[:6]]
    assert lines == sorted(lines) and first < lines[0] and lines[-1] < first + 20 and len(set(lines)) == 6
    assert [e.site for e in h.edges[6:]] == [e.site for e in h.edges[:6]]
    assert h.pairs(step=1) == [(e.site, e.kind) for e in h.edges[:6]]


def test_a_join_in_the_next_step_is_still_a_join():
    m = Machine(NAMES)
    with harness(m) as h:
        nested(m, h, prefetch=True)
    assert [(e.step, e.ordinal, e.a, e.b, e.kind) for e in h.edges][-1] == (2, 0, "main", "teacher", "join")


def test_a_child_seen_under_a_warmup_stream_is_reparented():
    m = Machine(("main", "warmup", "text"))
    with harness(m) as h:
        h.begin_step()
        m.warmup.wait_stream(m.main)
        m.text.wait_stream(m.warmup)
        m.warmup.wait_stream(m.text)
        m.main.wait_stream(m.warmup)
        h.begin_step()
        m.text.wait_stream(m.main)
        m.main.wait_stream(m.text)
    assert [e.kind for e in h.edges] == ["fork", "fork", "join", "join", "fork", "join"]


def test_outside_the_with_nothing_is_logged_and_the_method_is_put_back():
    orig = FakeStream.wait_stream
    m = Machine(NAMES)
    with harness(m, sc.late("all"), sleep_ms=5.0) as h:
        assert FakeStream.wait_stream is not orig
    assert FakeStream.wait_stream is orig
    nested(m, h)
    assert not h.edges and not h.sleeps and all(op != "sleep" for _, op, _ in m.trace)


def _ops(m):
    """What each queue holds, before it is drained: 'r' record, 'w' wait, 'S' sleep."""
    return {s.name: "".join({"record": "r", "wait": "w", "sleep": "S", "run": "k"}[op[0]] for op in s.q) for s in m.streams}


def _queued(schedule, **kw):
    m = Machine(NAMES)
    seen = {}
    m.drain = lambda: seen.update(_ops(m))                # look at the queues instead of running them
    with harness(m, schedule, sleep_ms=7.0, **kw) as h:
        nested(m, h)
    return seen, h


def test_every_schedule_queues_its_sleep_where_it_says():
    # no delay: the bare edges.  teacher: waits main, is recorded for teacher_text, waits teacher_text, is recorded for main
    base, h = _queued(None)
    assert base == {"main": "rwrw", "teacher": "wrwr", "teacher_text": "wr", "text": "wr"} and not h.sleeps
    # late(X): on X, right behind the wait of its fork
    seen, h = _queued(sc.late("teacher"))
    assert seen == {**base, "teacher": "wSrwr"} and h.sleeps == [(1, 0, "teacher", "after")]
    seen, h = _queued(sc.late("teacher_text"))
    assert seen == {**base, "teacher_text": "wSr"} and h.sleeps == [(1, 1, "teacher_text", "after")]
    seen, h = _queued(sc.late("text"))
    assert seen == {**base, "text": "wSr"} and h.sleeps == [(1, 4, "text", "after")]
    seen, h = _queued(sc.late("all"))
    assert seen == {"main": "rwrw", "teacher": "wSrwr", "teacher_text": "wSr", "text": "wSr"} and h.injected_ms == 21.0
    # late(main): on the PARENT, right behind the record its child waits for — main twice, and teacher as teacher_text's parent
    seen, h = _queued(sc.late("main"))
    assert seen == {"main": "rSwrSw", "teacher": "wrSwr", "teacher_text": "wr", "text": "wr"}
    assert h.sleeps == [(1, 0, "main", "after"), (1, 1, "teacher", "after"), (1, 4, "main", "after")]
    # head(main): one sleep in front of everything the step queues on the current stream
    seen, h = _queued(sc.head_main())
    assert seen == {**base, "main": "Srwrw"} and h.sleeps == [(1, -1, "main", "head")]
    with pytest.raises(ValueError):
        sc.late("main", "text")
    assert sc.count_sleeps(h.edges, sc.late("all")) == 3 and sc.count_sleeps(h.edges, sc.late("main")) == 3
    assert sc.count_sleeps(h.edges, sc.head_main(), steps=3) == 3


def test_drop_removes_exactly_one_edge():
    base, _ = _queued(None)
    seen, h = _queued(None, drop=[3])                    # main's join of the teacher
    assert seen == {**base, "main": "rrw", "teacher": "wrw"}       # one wait and the one record behind it
    assert [e.ordinal for e in h.edges if e.dropped] == [3] and len(h.edges) == 6      # still logged, still classified
    assert [e.kind for e in h.edges] == ["fork", "fork", "join", "join", "fork", "join"]
    site = h.edges[3].site
    seen, h = _queued(None, drop_sites=[site])           # the same edge by its call site
    assert seen == {**base, "main": "rrw", "teacher": "wrw"} and [e.ordinal for e in h.edges if e.dropped] == [3]
    seen, h = _queued(None, drop=[3], drop_steps=[2])    # another step's: nothing is dropped in step 1
    assert seen == base and not any(e.dropped for e in h.edges)


def test_nothing_is_injected_while_capturing():
    m = Machine(NAMES)
    seen = {}
    m.drain = lambda: seen.update(_ops(m))
    m.capturing_now = True
    with harness(m, sc.Schedule("everything", lambda e: [(e.a, "before"), (e.b, "after")], head=True), sleep_ms=7.0, drop=[0]) as h:
        nested(m, h)
    assert seen == {"main": "rwrw", "teacher": "wrwr", "teacher_text": "wr", "text": "wr"}
    assert not h.sleeps and h.injected_ms == 0.0 and all(e.capturing and not e.dropped for e in h.edges)
    assert h.pairs(capturing=False) == [] and len(h.pairs(capturing=True)) == 6
    # a capture runs on a stream of its own, which hangs from no attribute: it is called `capture`, only while capturing
    for capturing, want in ((True, "capture"), (False, "unknown")):
        m = Machine(NAMES)
        m.capturing_now = capturing
        with sc.StreamHarness(None, namer=lambda s, site: "unknown" if s.name == "main" else s.name, backend=m, product_root=HERE) as h:
            m.text.wait_stream(m.main)
            m.main.wait_stream(m.text)
        assert [(e.a, e.b, e.kind) for e in h.edges] == [("text", want, "fork"), (want, "text", "join")]


# ------------------------------------------------------------------------------------------------ sleeps, sites, checker

def test_sleep_sizes():
    assert sc.sleep_ms_for(0.1) == 1.0 and sc.sleep_ms_for(4.0) == 8.0 and sc.sleep_ms_for(400.0) == 50.0
    assert sc.sleep_ms_for(20.0, sleeps=9) == 40.0
    assert sc.sleep_ms_for(20.0, sleeps=38) == 25.0                  # 38 sleeps share 0.95 s
    assert 38 * sc.sleep_ms_for(20.0, sleeps=38) <= sc.BUDGET_MS


def test_every_wait_stream_of_the_product_has_a_name():
    sites = sc.find_sites()
    assert len(sites) == 12 and len(set(sites.values())) == 12
    for name, site in sites.items():
        fname, line = site.split(":")
        with open(os.path.join(sc.PRODUCT, fname), encoding="utf-8") as f:
            assert ".wait_stream(" in f.read().split("\n")[int(line) - 1], name
    ln = {k: int(v.split(":")[1]) for k, v in sites.items()}
    assert ln["teacher_fork_prefetch"] < ln["teacher_join_prefetched"] < ln["teacher_fork_beside"] < ln["teacher_join_beside"] \
        < ln["text_fork"] < ln["text_join"]


def test_the_checker_compares_words():
    nan = torch.tensor([1.0, float("nan"), -0.0])
    sc.assert_same_bits({"x": nan.clone()}, {"x": nan})                            # a NaN equals itself here
    with pytest.raises(sc.BitsDiffer, match="first differing tensor x, element 2 of 3"):
        sc.assert_same_bits({"x": torch.tensor([1.0, float("nan"), 0.0])}, {"x": nan})      # and -0.0 is not 0.0
    other_nan = nan.clone()
    other_nan.view(torch.int32)[1] ^= 1
    with pytest.raises(sc.BitsDiffer, match="element 1"):
        sc.assert_same_bits({"x": other_nan}, {"x": nan})
    a = {"p": torch.ones(3), "q": torch.arange(4, dtype=torch.bfloat16), "r": torch.zeros(2)}
    b = {k: v.clone() for k, v in a.items()}
    b["q"][3] += 1
    b["r"][0] = 1
    with pytest.raises(sc.BitsDiffer, match="first differing tensor q, element 3"):
        sc.assert_same_bits(b, a)
    assert sc.differing(b, a) == ["q", "r"]
    with pytest.raises(sc.BitsDiffer, match="names differ"):
        sc.assert_same_bits({"p": a["p"]}, a)
    with pytest.raises(sc.BitsDiffer, match="p: "):
        sc.assert_same_bits({**a, "p": torch.ones(3, dtype=torch.float64)}, a)
    with pytest.raises(sc.BitsDiffer, match="one side is None"):
        sc.assert_same_bits({**a, "p": None}, a)


def test_the_one_exception_is_bounded():
    """The `tok` gradient of a trainable text tower: float atomics, c * 2^-24 * sum|dx| per element (schedule_checks)."""
    from tests.schedule_checks import embed_atomic_bound
    ids = torch.tensor([[1, 2, 2], [2, 0, 1]])
    dx = torch.randn(2, 3, 4, generator=torch.Generator().manual_seed(0))
    bound = embed_atomic_bound(ids, dx, vocab=4)
    want = torch.zeros(4, 4).index_add_(0, ids.reshape(-1), dx.reshape(-1, 4))
    got = torch.zeros(4, 4).index_add_(0, ids.reshape(-1).flip(0), dx.reshape(-1, 4).flip(0))       # another order
    sc.assert_same_bits({"tok": got}, {"tok": want}, exceptions={"tok": bound})
    bad = got.clone()
    bad[3, 0] = 1e-6                                       # an id never met: the bound is 0 there
    with pytest.raises(sc.BitsDiffer, match="tok: outside its bound at 12"):
        sc.assert_same_bits({"tok": bad}, {"tok": want}, exceptions={"tok": bound})
    bad = got.clone()
    bad[2, 1] = float("nan")
    with pytest.raises(sc.BitsDiffer, match="outside its bound"):
        sc.assert_same_bits({"tok": bad}, {"tok": want}, exceptions={"tok": bound})


def test_a_pooled_stream_that_equals_a_known_one_keeps_its_own_name():
    """torch hands streams out of a pool, so a warm-up or capture stream can BE the queue of a long-lived stream and compare
    equal to it.  module_namer goes by identity, then main, then what hangs from nothing, and only then by value."""
    import types

    class S:
        def __init__(self, queue):
            self.queue = queue

        def __eq__(self, other):
            return isinstance(other, S) and other.queue == self.queue

        __hash__ = None

    main, text, teacher = S(0), S(5), S(6)
    mod = types.SimpleNamespace(_text_stream=text, _teacher_stream=teacher, teacher=types.SimpleNamespace(_text_side_stream=None))
    name = sc.module_namer(mod, main=main, extra={"wgrad": lambda: S(7)})
    assert name(text, "CLIP_image_distillation.py:1") == "text" and name(S(0), "engine.py:1") == "main"
    assert name(S(6), "patch_text_aggregation.py:1") == "teacher"        # torch.cuda.current_stream(): a new object, by value
    assert name(S(7), "engine.py:1") == "wgrad" and name(S(9), "engine.py:1") == "unknown"
    # the warm-up stream on the weight-gradient stream's queue, and on the text stream's: still the warm-up stream — at its own
    # call site and, from then on, as the current stream of the warm-up's steps
    for alias in (7, 5):
        name = sc.module_namer(mod, main=main, extra={"wgrad": lambda: S(7)})
        warm = S(alias)
        assert name(warm, "graph.py:33") == "warmup"
        assert name(S(alias), "CLIP_image_distillation.py:420") == "warmup"
        assert name(text, "CLIP_image_distillation.py:420") == "text"                # the attribute itself: identity wins
        # a capture's stream on a known queue: `capture` while capturing
        assert name(S(alias), "CLIP_image_distillation.py:420", True) == "capture"
        assert name(text, "CLIP_image_distillation.py:420", True) == "text" and name(S(0), "graph.py:39", True) == "main"
    # and through the harness: the log of a warm-up whose stream equals the weight-gradient stream's
    m = Machine(("main", "warmup", "text"))
    ids = {"main": main, "warmup": S(7), "text": text}
    name = sc.module_namer(mod, main=main, extra={"wgrad": lambda: S(7)})
    with sc.StreamHarness(None, namer=lambda s, site: name(ids[s.name], "graph.py:33" if s.name == "warmup" and not h.edges else "x.py:1"),
                          backend=m, product_root=HERE) as h:
        m.warmup.wait_stream(m.main)
        m.text.wait_stream(m.warmup)
        m.warmup.wait_stream(m.text)
        m.main.wait_stream(m.warmup)
    assert [(e.a, e.b, e.kind) for e in h.edges] == [("warmup", "main", "fork"), ("text", "warmup", "fork"),
                                                     ("warmup", "text", "join"), ("main", "warmup", "join")]
