"""Stream ordering of the training step under shifted timing (harness and checker: tests/stream_checks.py).

Every route of the step that uses a second stream — the frozen student text tower, the meta-teacher beside the student and
prefetched across steps, the teacher's own text tower, the weight-gradient stream of the token-major 16-bit backward — is run
three steps from a freshly built module (empty weight-copy caches), with a FusedAdamW step between them:
  * on ONE stream (every second stream switched off): the reference;
  * on its streams as they come: must equal the reference bit for bit, and the edge log must be the route's, exactly;
  * with a device-side sleep queued behind every fork of one side stream, of all of them, and on the parent: the same.
Then the host-ahead cases (one sleep at the head of every step, nothing synchronised until the end), and the controls: one edge
left out under the schedule made for it must CHANGE a result — the proof that the sleeps are long enough on this card."""
import argparse
import contextlib
import dataclasses
import logging
import os

import pytest
import torch

from dclip_amd import config as dcfg, synth
from tests import stream_checks as sc

pytestmark = pytest.mark.gpu

ONE_STREAM = {"DCLIP_TEXT_STREAM": "0", "DCLIP_TEACHER_STREAM": "0", "DCLIP_TEACHER_PREFETCH": "0",
              "DCLIP_TEACHER_TEXT_STREAM": "0", "DCLIP_BF16_WGRAD_STREAM": "0"}
STREAMS_ON = {k: "1" for k in ONE_STREAM}
SITES = sc.find_sites()
SITE_NAME = {v: k for k, v in SITES.items()}
STEPS = 3
TOTAL = {"ms": 0.0, "runs": 0}


def _dev():
    return torch.device("cuda:0")


@contextlib.contextmanager
def _env(values):
    old = {k: os.environ.get(k) for k in values}
    os.environ.update(values)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module", autouse=True)
def _report():
    sc.torch_backend().cycles_per_ms()            # calibrated before any run: it synchronises
    print(f"\n[stream order] torch.cuda._sleep: {sc.torch_backend().cycles_per_ms():.0f} cycles per ms")
    yield
    print(f"\n[stream order] injected sleep of the whole file: {TOTAL['ms']:.0f} ms in {TOTAL['runs']} delayed runs")
    for name, u in sorted(_UNDELAYED.items()):
        print(f"[stream order] {name}: undelayed step {u.step_ms:.2f} ms, sleep {sc.sleep_ms_for(u.step_ms):.1f} ms")


# ------------------------------------------------------------------------------------------------ modules and batches

_KEPT = {}


def _kept(key, make):
    """Host-side inputs that are made once and never written: state dicts and batches (a module is always built afresh)."""
    if key not in _KEPT:
        _KEPT[key] = make()
    return _KEPT[key]


def _state_dict(cfg, seed, gain):
    return _kept(("sd", cfg.name, seed, gain), lambda: synth.synth_clip_state_dict(cfg, seed=seed, gain=gain))


def _hp(B):
    return argparse.Namespace(learning_rate=1e-3, warmup_steps=0, total_steps=100, train_batch_size=B, eval_batch_size=B)


def _meta_module(precision="fp32", own_teacher_clip=True, tower_precision="fp32", packed_text=False, cfg=None):
    """test_teacher_prefetch_gpu._module, with the teacher's tower precision, packed_text and the widths as arguments."""
    from dclip_amd.clip_model import from_hf_state_dict
    from dclip_amd.CLIP_image_distillation import CLIPImageDistillation
    from dclip_amd.patch_text_aggregation import PatchTextAggregation
    dev, cfg = _dev(), cfg or dcfg.tiny()
    student = from_hf_state_dict(cfg, _state_dict(cfg, 0, 3.0), device=dev)
    E = cfg.projection_dim
    tclip = student
    if own_teacher_clip:
        tclip = from_hf_state_dict(cfg, _state_dict(cfg, 7, 3.0), device=dev)
        for p in tclip.parameters():
            p.requires_grad_(False)
    teacher = PatchTextAggregation(embed_dim=E, num_heads=max(E // 64, 1), clip_model=tclip, tower_precision=tower_precision)
    teacher.load_state_dict({f"cross_modal_attention.{k}": v for k, v in synth.synth_cross_modal_state_dict(E, seed=31).items()})
    mod = CLIPImageDistillation(_hp(4), student, None, teacher=teacher.to(dev), freeze_mode="north_star",
                                student_precision=precision, packed_text=packed_text).to(dev)
    return mod, cfg


def _meta_batches(cfg, n, max_tokens=True, text_lens=False, device=True, counts=True):
    from tests.test_teacher_prefetch_gpu import _batches
    out = _batches(cfg, n, B=4, R=3, device=_dev() if device else None)
    for b in out:
        if not counts:
            b.pop("region_counts")
        if max_tokens:
            b["max_tokens"] = cfg.text.max_position_embeddings - 2
        if text_lens:
            from dclip_amd.clip_model import packed_text_tables
            b["text_lens"] = packed_text_tables(b["input_ids"].cpu(), cfg.text.eos_token_id)["lens"]
    return out


def _targets_module(cfg, precision="fp32", B=6, seed=0, gain=3.0):
    """A student with given targets (no teacher pass): the frozen text tower is the only second stream of the forward."""
    from dclip_amd.clip_model import from_hf_state_dict
    from dclip_amd.CLIP_image_distillation import CLIPImageDistillation
    dev = _dev()
    student = from_hf_state_dict(cfg, _state_dict(cfg, seed, gain), device=dev)
    return CLIPImageDistillation(_hp(B), student, None, freeze_mode="north_star", student_precision=precision).to(dev)


def _targets_batches(cfg, n, B, device=True, pinned=False):
    out = []
    for i in range(n):
        b = {"pixel_values": synth.synth_pixel_values(B, cfg.vision, seed=i),
             "input_ids": synth.synth_input_ids(B, cfg.text, seed=100 + i, ragged=True),
             "teacher_image_emb": synth.synth_embeddings(B, cfg.projection_dim, seed=200 + i),
             "teacher_text_emb": synth.synth_embeddings(B, cfg.projection_dim, seed=300 + i)}
        if device:
            b = {k: v.to(_dev()) for k, v in b.items()}
        elif pinned:
            b = {k: v.pin_memory() for k, v in b.items()}
        out.append(b)
    return out


def _wide_meta_batches(cfg, n, B, R=2):
    out = []
    for k in range(n):
        out.append({"pixel_values": synth.synth_pixel_values(B, cfg.vision, seed=10 + k).to(_dev()),
                    "input_ids": synth.synth_input_ids(B, cfg.text, seed=20 + k, ragged=True, min_len=5).to(_dev()),
                    "regions": synth.synth_regions(B, R, cfg.vision, seed=30 + k).to(_dev()),
                    "region_counts": torch.tensor([R, 1, 2, 0][:R + 2] * B)[:B].clamp(max=R),
                    "max_tokens": cfg.text.max_position_embeddings - 2})
    return out


def _wide_cfg():
    from tests.test_schedule_grads_gpu import WIDE              # §26's wide2: ViT-B/32 widths, two layers, 9600 tokens at B = 192
    return WIDE.config(), WIDE.B


# ------------------------------------------------------------------------------------------------ cases

@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    build: object                     # () -> (module, batches)
    streams: tuple                    # the side streams expected in the log
    log: object                       # step (1-based) -> [(site name, kind)] expected
    driver: str = "steps"             # "steps" | "fit" | "validation"
    prefetch: bool = False
    steps: int = STEPS


def _text_pair():
    return [("text_fork", "fork"), ("text_join", "join")]


def _teacher_text_pair():
    return [("teacher_text_fork", "fork"), ("teacher_text_join", "join")]


def _log_targets(step):
    return _text_pair()


def _log_meta(last, text=True, prefetch=True):
    """The meta-teacher step.  Step 1 runs its teacher beside the student; with the pipelined teacher every step but the last
    starts the next batch's teacher behind its forward, and every step but the first joins the one started for it."""
    def log(step):
        if step == 1 or not prefetch:
            out = [("teacher_fork_beside", "fork")] + _teacher_text_pair() + [("teacher_join_beside", "join")]
        else:
            out = [("teacher_join_prefetched", "join")]
        out += _text_pair() if text else []
        if prefetch and step < last:
            out += [("teacher_fork_prefetch", "fork")] + _teacher_text_pair()
        return out
    return log


def _log_validation(step):
    """Two training steps (the second one's teacher pipelined), then a validation step, which runs its teacher beside."""
    return _log_meta(2)(step) if step < 3 else _log_meta(1, prefetch=False)(step)


def _log_wgrad(layers, text=True, head=()):
    def log(step):
        out = list(head) + (_text_pair() if text else [])
        for _ in range(layers):
            out += [("wgrad_fork", "fork")] * 4 + [("wgrad_join", "join")]
        return out
    return log


def _build_targets(precision="fp32", wide=False):
    def build():
        cfg, B = _wide_cfg() if wide else (dcfg.tiny(), 6)
        return _targets_module(cfg, precision, B), _kept(("targets", cfg.name, B), lambda: _targets_batches(cfg, STEPS, B))
    return build


def _build_meta(n=STEPS, max_tokens=True, text_lens=False, counts=True, **kw):
    def build():
        mod, cfg = _meta_module(**kw)
        return mod, _kept(("meta", n, max_tokens, text_lens, counts),
                          lambda: _meta_batches(cfg, n, max_tokens=max_tokens, text_lens=text_lens, counts=counts))
    return build


def _build_wide_meta():
    cfg, B = _wide_cfg()
    mod, _ = _meta_module(precision="bf16", tower_precision="bf16", cfg=cfg)
    return mod, _kept(("wide_meta", B), lambda: _wide_meta_batches(cfg, STEPS, B))


def _log_wide_meta(step):
    """_log_meta with the two layers' weight-gradient forks and joins where the backward runs: behind the forward's edges and
    in front of the next batch's teacher... which the driver starts BEFORE the backward."""
    out = _log_meta(STEPS)(step)
    for _ in range(2):
        out += [("wgrad_fork", "fork")] * 4 + [("wgrad_join", "join")]
    return out


T3 = ("text", "teacher", "teacher_text")
CASES = [
    Case("fp32_targets", _build_targets(), ("text",), _log_targets),
    Case("meta_max_tokens", _build_meta(), T3, _log_meta(STEPS), prefetch=True),
    Case("meta_host_sync", _build_meta(max_tokens=False), T3, _log_meta(STEPS), prefetch=True),
    # host-side `region_counts` go to the device in a blocking copy on the teacher's stream and `max_tokens` not given is a read
    # of `eos`: either way the host waits for the teacher's queue in the middle of the teacher.  Without both the host never
    # waits — the form in which a teacher that runs late is really behind the main stream (the controls use it)
    Case("meta_no_host_wait", _build_meta(counts=False), T3, _log_meta(STEPS), prefetch=True),
    Case("meta_fit", _build_meta(n=4), T3, _log_meta(4), driver="fit", prefetch=True, steps=4),
    # one model's caches under teacher and student: the pipelined teacher is refused (it would read weights being trained), and
    # the teacher's text pass serves the student's text features — no `text` stream on this route
    Case("meta_shared_clip", _build_meta(own_teacher_clip=False), ("teacher", "teacher_text"),
         _log_meta(STEPS, text=False, prefetch=False), prefetch=True),
    Case("meta_packed_text", _build_meta(text_lens=True, packed_text=True), T3, _log_meta(STEPS), prefetch=True),
    Case("wide2_bf16", _build_targets("bf16", wide=True), ("text", "wgrad"), _log_wgrad(2)),
    Case("wide2_fp16", _build_targets("fp16", wide=True), ("text", "wgrad"), _log_wgrad(2)),
    Case("c3_tiny_bf16", _build_meta(precision="bf16", tower_precision="bf16"), T3, _log_meta(STEPS), prefetch=True),
    # the tiny widths never reach the token-major backward (its plan refuses D = 128 at any batch), so the weight-gradient stream
    # is not in c3_tiny's log: all FOUR side streams of one step need §26's wide2 under the meta-teacher
    Case("c3_wide2_bf16", _build_wide_meta, T3 + ("wgrad",), _log_wide_meta, prefetch=True),
    Case("meta_validation", _build_meta(), T3, _log_validation, driver="validation", prefetch=True),
]
CASE = {c.name: c for c in CASES}


def _schedules(case):
    return ["none"] + [f"late({s})" for s in case.streams] + ["late(all)", "late(main)"]


def _schedule(label):
    if label == "none":
        return sc.no_delay()
    return sc.late(*label[5:-1].split(","))


# ------------------------------------------------------------------------------------------------ running a case

@dataclasses.dataclass
class Run:
    out: dict
    harness: object
    step_ms: float


def _snapshot(out, tag, mod, loss, with_grads=True, with_params=False):
    out[f"{tag}.loss"] = loss.detach().clone()
    for k, v in mod.last_losses.items():
        out[f"{tag}.{k}"] = v.clone()
    if with_grads:
        for n, p in mod.named_parameters():
            if p.grad is not None:
                out[f"{tag}.grad.{n}"] = p.grad.clone()
    if with_params:
        for n, p in mod.named_parameters():
            if p.requires_grad:
                out[f"{tag}.param.{n}"] = p.detach().clone()


def _drive_steps(case, mod, batches, h, out, marks, validation=False):
    from dclip_amd.optim import FusedAdamW
    opt = FusedAdamW([p for p in mod.parameters() if p.requires_grad], lr=1e-3)
    train = len(batches) - 1 if validation else len(batches)
    for i in range(train):
        marks.append(torch.cuda.Event(enable_timing=True))
        marks[-1].record()
        h.begin_step()
        loss = mod.training_step(batches[i])
        if case.prefetch and i + 1 < train:
            h.prefetched.append(mod.prefetch_teacher(batches[i + 1]))
        loss.backward()
        _snapshot(out, f"s{i}", mod, loss)
        opt.step()
        _snapshot(out, f"s{i}", mod, loss, with_grads=False, with_params=True)
        mod.zero_grad(set_to_none=True)
    if validation:
        marks.append(torch.cuda.Event(enable_timing=True))
        marks[-1].record()
        h.begin_step()
        mod.eval()
        with torch.no_grad():
            loss = mod.validation_step(batches[train])
        _snapshot(out, "val", mod, loss, with_grads=False)


def _drive_fit(case, mod, batches, h, out, marks):
    from dclip_amd.lightning_lite import Trainer
    real, k = mod.training_step, [0]

    def step(batch, *a):
        marks.append(torch.cuda.Event(enable_timing=True))
        marks[-1].record()
        h.begin_step()
        loss = real(batch, *a)
        _snapshot(out, f"s{k[0]}", mod, loss, with_grads=False)
        k[0] += 1
        return loss

    mod.training_step = step
    Trainer(max_epochs=1, accelerator="gpu", devices=1, gradient_clip_val=0.5, accumulate_grad_batches=1,
            enable_progress_bar=False, logger=False, enable_checkpointing=False).fit(mod, batches, None)
    for n, p in mod.named_parameters():
        if p.requires_grad:
            out[f"end.param.{n}"] = p.detach().clone()


def run_case(case, schedule=None, sleep_ms=0.0, one_stream=False, drop=(), drop_steps=None):
    """Build the case's module afresh and run it.  No synchronisation between the first launch and the end."""
    with _env(ONE_STREAM if one_stream else STREAMS_ON):
        torch.cuda.synchronize()
        mod, batches = case.build()
        main = torch.cuda.current_stream()
        out, marks = {}, []
        with sc.StreamHarness(schedule, sc.module_namer(mod, main=main), drop=drop, drop_steps=drop_steps, sleep_ms=sleep_ms) as h:
            h.prefetched = []
            if case.driver == "fit":
                _drive_fit(case, mod, batches, h, out, marks)
            else:
                _drive_steps(case, mod, batches, h, out, marks, validation=case.driver == "validation")
            end = torch.cuda.Event(enable_timing=True)
            end.record()
        torch.cuda.synchronize()
        marks.append(end)
        times = sorted(a.elapsed_time(b) for a, b in zip(marks, marks[1:]))
        mod._prefetched = None
    TOTAL["ms"] += h.injected_ms
    TOTAL["runs"] += int(h.injected_ms > 0)
    return Run(out, h, times[len(times) // 2])


_REFERENCE, _UNDELAYED = {}, {}


def reference(case):
    if case.name not in _REFERENCE:
        r = run_case(case, one_stream=True)
        assert not r.harness.edges, f"{case.name}: the one-stream reference met a wait_stream:\n{r.harness.describe()}"
        _REFERENCE[case.name] = r
    return _REFERENCE[case.name]


def undelayed(case):
    if case.name not in _UNDELAYED:
        _UNDELAYED[case.name] = run_case(case)
    return _UNDELAYED[case.name]


def assert_route(case, h):
    """The edge log holds exactly the route's (site, kind) pairs, step by step, and names exactly its streams."""
    for step in range(1, case.steps + 1):
        got = [(SITE_NAME.get(site, site), kind) for site, kind in h.pairs(step=step)]
        assert got == case.log(step), f"{case.name} step {step}: the edge log is\n{h.describe()}"
    assert len(h.edges) == sum(len(case.log(s)) for s in range(1, case.steps + 1)), h.describe()
    assert h.streams_seen() == {"main", *case.streams}, (case.name, h.streams_seen())


# ------------------------------------------------------------------------------------------------ the routes

@pytest.mark.parametrize("name,label", [(c.name, s) for c in CASES for s in _schedules(c)])
def test_route_is_bit_equal_to_one_stream(name, label):
    case = CASE[name]
    ref, base = reference(case), undelayed(case)
    if label == "none":
        assert_route(case, base.harness)
        sc.assert_same_bits(base.out, ref.out, what=f"{name}, streams as they come")
        assert base.harness.injected_ms == 0.0 and len(ref.out) > 10
        if case.driver != "fit":
            # started wherever the teacher reads nothing that is being trained; refused on one model's shared towers
            started = case.prefetch and name != "meta_shared_clip"
            assert base.harness.prefetched == ([started] * len(base.harness.prefetched)) and not any(ref.harness.prefetched)
            assert len(base.harness.prefetched) == (case.steps - (2 if case.driver == "validation" else 1) if case.prefetch else 0)
        return
    sched = _schedule(label)
    n = sc.count_sleeps(base.harness.edges, sched)
    assert n > 0, f"{name}: {label} has no fork to sleep behind"
    ms = sc.sleep_ms_for(base.step_ms, n)
    got = run_case(case, sched, ms)
    print(f"[stream order] {name} {label}: step {base.step_ms:.2f} ms, {n} sleeps of {ms:.1f} ms")
    assert len(got.harness.sleeps) == n and got.harness.injected_ms <= sc.BUDGET_MS
    assert_route(case, got.harness)
    sc.assert_same_bits(got.out, ref.out, what=f"{name} under {label}")


# ------------------------------------------------------------------------------------------------ host ahead of the device

def _loader(batches, h, sync, dev_copy=True):
    """Batches for Trainer.fit.  `sync`: the run that synchronises after every step.  Otherwise the harness's head sleep goes
    onto the main stream and the batch is copied into its device tensors BEHIND it (non-blocking, from pinned memory): the
    host is ahead of the device by the sleep when the step's launches begin."""
    for b in batches:
        if sync:
            torch.cuda.synchronize()
        else:
            h.begin_step()
        yield {k: (v.to(_dev(), non_blocking=True) if dev_copy and isinstance(v, torch.Tensor) and v.is_pinned() else v)
               for k, v in b.items()} if dev_copy else b


def _fit_host_ahead(build, trainer_kw, sync, sleep_ms=0.0, dev_copy=True, scaler=None):
    from dclip_amd.lightning_lite import Trainer
    with _env(STREAMS_ON):
        torch.cuda.synchronize()
        mod, batches = build()
        box, conf = {}, mod.configure_optimizers

        def keep():
            opts, scheds = conf()
            box["opt"] = opts[0]
            return opts, scheds
        mod.configure_optimizers = keep
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        sched = sc.no_delay() if sync else sc.head_main()
        with sc.StreamHarness(sched, sc.module_namer(mod, main=torch.cuda.current_stream()), sleep_ms=sleep_ms) as h:
            e0.record()
            Trainer(max_epochs=1, accelerator="gpu", devices=1, gradient_clip_val=0.5, enable_progress_bar=False, logger=False,
                    enable_checkpointing=False, loss_scaler=scaler, **trainer_kw).fit(mod, _loader(batches, h, sync, dev_copy), None)
            e1.record()
            # how far the host is ahead when fit returns, read without waiting: is the device still busy, and how many of the
            # optimizer's four staging buffers still wait for their upload (the events FusedAdamW._records guards them with)
            ring = box["opt"]._table.get(0, {}).get("done", [])
            h.lead = {"ahead": not e1.query(), "ring_pending": sum(1 for ev in ring if ev is not None and not ev.query())}
        torch.cuda.synchronize()
        mod._prefetched = None
    out = {f"param.{n}": p.detach().clone() for n, p in mod.named_parameters() if p.requires_grad}
    TOTAL["ms"] += h.injected_ms
    TOTAL["runs"] += int(h.injected_ms > 0)
    return out, h, box["opt"], (e0.elapsed_time(e1) / len(batches), len(batches)), mod


def _pinned(batches):
    return [{k: (v.cpu().pin_memory() if isinstance(v, torch.Tensor) and k != "region_counts" else v) for k, v in b.items()}
            for b in batches]


def _host_ahead_pair(build, trainer_kw, dev_copy=True, scalers=(None, None)):
    want, _, opt_w, (step_ms, n), _ = _fit_host_ahead(build, trainer_kw, sync=True, dev_copy=dev_copy, scaler=scalers[0])
    ms = sc.sleep_ms_for(step_ms, n)
    got, h, opt_g, _, mod = _fit_host_ahead(build, trainer_kw, sync=False, sleep_ms=ms, dev_copy=dev_copy, scaler=scalers[1])
    print(f"[stream order] host ahead: step {step_ms:.2f} ms, {n} head sleeps of {ms:.1f} ms; when fit returned: {h.lead}")
    assert len(h.sleeps) == n and all(s[3] == "head" and s[2] == "main" for s in h.sleeps) and h.injected_ms <= sc.BUDGET_MS
    return got, want, opt_g, opt_w, h, mod


FIT6 = dict(accumulate_grad_batches=2, lr_interval="step")


def test_host_ahead_eager_trainer_passes_the_staging_ring():
    """6 optimizer steps over 12 micro-batches (the ring has 4 staging buffers), the pipelined meta-teacher beside them.  The
    batches carry `max_tokens` and NO host-side `region_counts` (those go to the device in a blocking copy inside the teacher, which
    would hold the host at every micro-batch): nothing in the loop waits for the device but the ring's own guard, and the host
    IS ahead when fit returns — the device still busy, staging buffers still waiting for their upload."""
    def build():
        mod, cfg = _meta_module()
        return mod, _pinned(_meta_batches(cfg, 12, device=False, counts=False))
    got, want, opt, _, h, mod = _host_ahead_pair(build, FIT6)
    assert mod.global_step == 6 and opt._table[0]["next"] == 6 % 4
    assert h.lead["ahead"] and h.lead["ring_pending"] >= 1, f"the host was not ahead of the device when fit returned: {h.lead}"
    assert {"text", "teacher", "teacher_text"} <= h.streams_seen()
    sc.assert_same_bits(got, want, what="eager trainer, host ahead")


@pytest.mark.parametrize("memory", ["pinned", "pageable"])
def test_host_ahead_graph_replay(memory):
    """GraphedStep.load copies into the captured buffers (non-blocking only from pinned memory) and replay follows at once."""
    cfg = dcfg.tiny()

    def build():
        b = _targets_batches(cfg, 12, 4, device=False, pinned=memory == "pinned")
        for x in b:
            x.pop("teacher_text_emb")
        return _targets_module(cfg, B=4), b
    got, want, _, _, h, mod = _host_ahead_pair(build, dict(use_hip_graph=True, **FIT6), dev_copy=False)
    assert mod.global_step == 6
    if memory == "pinned":           # (a copy from pageable memory blocks the host at every load: by design never ahead)
        assert h.lead["ahead"], f"the host was not ahead of the device when fit returned: {h.lead}"
    # the warm-up on its throwaway stream, then the capture: logged, classified, and nothing injected inside either
    names = [(SITE_NAME.get(e.site, e.site), e.kind, e.capturing) for e in h.edges]
    warm = [("text_fork", "fork", False), ("text_join", "join", False)]
    assert names == [("warmup_fork", "fork", False)] + warm * 2 + [("warmup_join", "join", False),
                                                                  ("text_fork", "fork", True), ("text_join", "join", True)], h.describe()
    assert {e.a for e in h.edges} | {e.b for e in h.edges} == {"main", "warmup", "text", "capture"}
    sc.assert_same_bits(got, want, what=f"graph replay from {memory} memory, host ahead")


def test_host_ahead_fp16_overflow_takes_the_adam_count_back():
    """An inf in one target of step 2: that step is skipped on the device, its Adam count is taken back at the next step's
    settle_scaled_step — parameters, every state's step and the scale equal the synchronised run's."""
    from dclip_amd.amp import DynamicLossScaler
    cfg = dcfg.tiny()

    def build():
        b = _targets_batches(cfg, 4, 4, device=False)
        b[1]["teacher_image_emb"][2, 5] = float("inf")
        return _targets_module(cfg, "fp16", B=4, seed=7, gain=4.0), [{k: v.pin_memory() for k, v in x.items()} for x in b]
    scalers = (DynamicLossScaler(init_scale=2.0 ** 8), DynamicLossScaler(init_scale=2.0 ** 8))
    got, want, opt_g, opt_w, h, mod = _host_ahead_pair(build, dict(accumulate_grad_batches=1, lr_interval="step"), scalers=scalers)
    sc.assert_same_bits(got, want, what="fp16 student, host ahead")
    steps_g = [int(v["step"]) for v in opt_g.state_dict()["state"].values()]
    steps_w = [int(v["step"]) for v in opt_w.state_dict()["state"].values()]
    assert steps_g == steps_w and len(steps_g) > 10 and set(steps_w) == {3}, (steps_g[:4], steps_w[:4])      # 4 steps, one skipped
    assert scalers[1].get_scale() == scalers[0].get_scale() == 2.0 ** 7


def test_host_ahead_split16_guard_flag(monkeypatch, caplog):
    """A LayerNorm gain of 1e7 before step 2 (as test_guard_flags_without_a_sync): the features of every step are bit-equal to
    the undelayed run's, and the flag — copied to pinned memory behind the refresh, never waited for — is seen at the next
    refresh that finds it landed: with the host ahead that is the first refresh after the device has caught up."""
    from dclip_amd import engine
    from dclip_amd.clip_model import from_hf_state_dict
    cfg = dcfg.tiny()
    sd = synth.synth_clip_state_dict(cfg, seed=5, gain=2.0)
    pix = synth.synth_pixel_values(4, cfg.vision, seed=1).to(_dev())
    probe = synth.synth_embeddings(4, cfg.projection_dim, seed=9).to(_dev())
    monkeypatch.setattr(engine, "_VSPLIT16", True)

    def run(sleep_ms, sync_each=False):
        monkeypatch.setattr(engine, "_SPLIT16_LOGGED", set())
        caplog.clear()
        model = from_hf_state_dict(cfg, sd, device=_dev())
        feats, first_seen = {}, None
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with caplog.at_level(logging.WARNING, logger="dclip_amd"), \
                sc.StreamHarness(sc.head_main(), sc.module_namer(None, main=torch.cuda.current_stream()), sleep_ms=sleep_ms) as h:
            e0.record()
            for i in range(4):
                h.begin_step()
                if i == 1:
                    with torch.no_grad():
                        for ln in (model.vision_model.encoder.layers[1].layer_norm1, model.vision_model.encoder.layers[1].layer_norm2):
                            ln.weight.fill_(1e7)
                if i > 1:
                    with torch.no_grad():
                        model.vision_model.encoder.layers[0].layer_norm1.bias.add_(0.0)       # a version bump: this forward refreshes
                for q in model.parameters():
                    q.grad = None
                feat = model.get_image_features(pixel_values=pix)
                if first_seen is None and any("layer flags" in r.getMessage() for r in caplog.records):
                    first_seen = i
                (feat * probe).sum().backward()
                feats[f"s{i}.features"] = feat.detach().clone()
                for n, p in model.named_parameters():
                    if p.grad is not None:
                        feats[f"s{i}.grad.{n}"] = p.grad.clone()
                if sync_each:
                    torch.cuda.synchronize()
            e1.record()
            torch.cuda.synchronize()
            with torch.no_grad():
                model.vision_model.encoder.layers[0].layer_norm1.bias.add_(0.0)
            model.get_image_features(pixel_values=pix)                                       # the next refresh after the device caught up
            torch.cuda.synchronize()
        msgs = [r.getMessage() for r in caplog.records if "layer flags" in r.getMessage()]
        TOTAL["ms"] += h.injected_ms
        TOTAL["runs"] += int(h.injected_ms > 0)
        assert model._vsplit16_cache().get("__vsplit16__") is not None, "the split-fp16 vision path did not run"
        return feats, msgs, first_seen, h, e0.elapsed_time(e1) / 4

    # the host in step with the device: the flag of step 1's refresh is seen at the NEXT refresh, step 2's
    synced, msgs_s, seen_s, _, _ = run(0.0, sync_each=True)
    assert seen_s == 2 and len(msgs_s) == 1 and "1:1" in msgs_s[0], (seen_s, msgs_s)
    want, msgs_w, _, _, step_ms = run(0.0)
    ms = sc.sleep_ms_for(step_ms, 4)                      # twice this case's own undelayed step
    got, msgs_g, seen_g, h, _ = run(ms)
    print(f"[stream order] guard flag: step {step_ms:.2f} ms, 4 head sleeps of {ms:.1f} ms; first seen at step {seen_g} "
          f"(None: after the device caught up)")
    assert len(h.sleeps) == 4 and h.injected_ms <= sc.BUDGET_MS
    assert len(msgs_w) == 1 and "1:1" in msgs_w[0], msgs_w
    # the host ahead: never before the refresh behind the flagged one, and logged exactly once whenever it is first seen
    assert (seen_g is None or seen_g >= 2) and len(msgs_g) == 1 and "1:1" in msgs_g[0], (seen_g, msgs_g)
    sc.assert_same_bits(got, want, what="split-fp16 guard, host ahead")
    sc.assert_same_bits(synced, want, what="split-fp16 guard, synchronised after every step")


# ------------------------------------------------------------------------------------------------ controls

def _control(case_name, site_name, sched_label, expect, prefetch=None, head_before_backward=False):
    """Two steps as they are, then a third with the edges at `site_name` left out under the schedule made for them: some tensor
    of that step must differ from the one-stream reference.  (The third step: a fresh module's first steps build caches, the
    optimizer's state and pinned staging on the host, which takes longer than any sleep here — the device would be idle and
    nothing could run late.)  Only edges across which nothing but floating-point data flows are ever left out:
    a stale read then yields wrong numbers from allocated memory, never a wrong address.  The run ends in a synchronize."""
    from dclip_amd import engine
    from dclip_amd.optim import FusedAdamW
    case = CASE[case_name]
    ref, base = reference(case), undelayed(case)
    prefetch = case.prefetch if prefetch is None else prefetch
    sched = sc.head_main() if head_before_backward else _schedule(sched_label)
    n = 1 if head_before_backward else sc.count_sleeps(base.harness.edges, sched)
    ms = sc.sleep_ms_for(base.step_ms, n)
    steps, last = STEPS, STEPS
    with _env(STREAMS_ON):
        torch.cuda.synchronize()
        mod, batches = case.build()
        opt = FusedAdamW([p for p in mod.parameters() if p.requires_grad], lr=1e-3)
        main = torch.cuda.current_stream()
        out = {}
        with _restored(engine._WGRAD_STREAMS, dict(engine._WGRAD_STREAMS)), \
                sc.StreamHarness(sched, sc.module_namer(mod, main=main), drop_sites=[SITES[site_name]], drop_steps=[last],
                                 sleep_ms=ms) as h:
            placed = _place_streams(mod, main)            # (probes: it synchronises; nothing of the run is queued yet)
            wgrad_used = engine._WGRAD_STREAMS.get(_dev().index)
            for i in range(steps):
                h.begin_step(head=not head_before_backward)
                loss = mod.training_step(batches[i])
                if prefetch and i + 1 < steps:
                    mod.prefetch_teacher(batches[i + 1])
                if head_before_backward and i + 1 == last:
                    h.head()
                loss.backward()
                if i + 1 == last:
                    _snapshot(out, f"s{i}", mod, loss)
                else:
                    opt.step()
                    mod.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
        mod._prefetched = None
        # which queues the card gave this run: a side stream that shares main's hardware queue cannot run late against it
        side = {"text": mod._text_stream, "teacher": mod._teacher_stream,
                "teacher_text": getattr(mod.teacher, "_text_side_stream", None), "wgrad": wgrad_used}
        beside = {k: sc.runs_beside(main, v) for k, v in side.items() if v is not None and k in case.streams}
    TOTAL["ms"] += h.injected_ms
    TOTAL["runs"] += 1
    dropped = [e for e in h.edges if e.dropped]
    assert dropped and all(e.step == last and e.site == SITES[site_name] for e in dropped) and h.injected_ms <= sc.BUDGET_MS
    tag = f"s{last - 1}."
    want = {k: v for k, v in ref.out.items() if k.startswith(tag) and ".param." not in k}
    differ = sc.differing({k: out[k] for k in want}, want)
    print(f"[stream order] control {case_name} without {site_name} x{len(dropped)} under {sched.name} ({len(h.sleeps)} sleeps of "
          f"{ms:.1f} ms; streams placed: {placed}; runs beside main: {beside}): {len(differ)} of {len(want)} tensors differ, first {differ[:3]}")
    assert any(expect(k[len(tag):]) for k in differ), \
        f"leaving out {site_name} under {sched.name} changed {differ[:5] or 'nothing'} (runs beside main: {beside})"


@contextlib.contextmanager
def _restored(d, old):
    try:
        yield
    finally:
        d.clear()
        d.update(old)


def _place_streams(mod, main):
    """Side streams for a control, chosen so that the stream whose edge is left out CAN run late against main: torch hands
    streams out of a pool that the runtime spreads over the process's 4 hardware queues, the main stream has one of them, and a
    side stream on main's queue is served in launch order — nothing on it is ever behind main.  (The cases take the streams the
    product makes; which queues those land on varies from run to run.)  Candidates are probed with sc.runs_beside."""
    from dclip_amd import engine
    cands = [torch.cuda.Stream(device=_dev()) for _ in range(8)]
    free = [c for c in cands if sc.runs_beside(main, c)]
    if len(free) < 3:
        return False
    teacher = free[0]
    others = [c for c in free[1:] if c != teacher and sc.runs_beside(teacher, c)]
    if len(others) < 2:
        return False
    mod._teacher_stream, mod._text_stream = teacher, others[1]
    if hasattr(mod.teacher, "_clip"):
        object.__setattr__(mod.teacher, "_text_side_stream", others[0])
    # the weight-gradient stream is one per process (engine._WGRAD_STREAMS), made by whichever test came first: the caller puts
    # the old one back
    engine._WGRAD_STREAMS[_dev().index] = others[2] if len(others) > 2 else others[0]
    return True


def _weight_grad(k):
    return k.startswith("grad.") and k.endswith("weight")


def test_control_wgrad_join():
    _control("wide2_bf16", "wgrad_join", "late(wgrad)", _weight_grad)


def test_control_student_text_join():
    _control("fp32_targets", "text_join", "late(text)", lambda k: k == "loss_text")


def test_control_teacher_join_beside():
    _control("meta_no_host_wait", "teacher_join_beside", "late(teacher)", lambda k: k == "loss_image", prefetch=False)


def test_control_teacher_join_prefetched():
    _control("meta_no_host_wait", "teacher_join_prefetched", "late(teacher)", lambda k: k == "loss_image")


def test_control_wgrad_fork():
    _control("wide2_bf16", "wgrad_fork", None, _weight_grad, head_before_backward=True)
