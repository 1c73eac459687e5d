"""Host-side pieces of bench.py that need no GPU: the `single_stream` bracket around event-sampled steps restores every
second-stream switch it turned off (module flags and the environment variables read at call time), whatever they were."""
import os
import types

import bench


def test_single_stream_switches_off_and_restores_every_second_stream(monkeypatch):
    mod = types.SimpleNamespace(overlap_teacher=None, overlap_frozen_text=True)
    monkeypatch.delenv("DCLIP_BF16_WGRAD_STREAM", raising=False)
    monkeypatch.setenv("DCLIP_TEACHER_TEXT_STREAM", "1")
    with bench.single_stream(mod):
        assert mod.overlap_teacher is False and mod.overlap_frozen_text is False
        assert os.environ["DCLIP_BF16_WGRAD_STREAM"] == "0" and os.environ["DCLIP_TEACHER_TEXT_STREAM"] == "0"
    assert mod.overlap_teacher is None and mod.overlap_frozen_text is True
    assert "DCLIP_BF16_WGRAD_STREAM" not in os.environ and os.environ["DCLIP_TEACHER_TEXT_STREAM"] == "1"
    with bench.single_stream(mod, on=False):                      # a step that is not sampled: nothing is touched
        assert mod.overlap_frozen_text is True and "DCLIP_BF16_WGRAD_STREAM" not in os.environ
    try:
        with bench.single_stream(mod):
            raise RuntimeError("step failed")
    except RuntimeError:
        pass
    assert mod.overlap_teacher is None and mod.overlap_frozen_text is True and "DCLIP_BF16_WGRAD_STREAM" not in os.environ


def test_step_flops_and_teacher_flops_are_positive_and_scale():
    from dclip_amd import config as dcfg
    b32, l14 = dcfg.vit_b32(), dcfg.vit_l14()
    T = b32.text.max_position_embeddings
    assert bench.step_flops_per_image(b32, T) > 0
    one = bench.meta_teacher_flops(b32, b32, 256, 8, T)
    assert bench.meta_teacher_flops(b32, b32, 512, 8, T) == 2 * one
    assert bench.meta_teacher_flops(b32, l14, 256, 8, T) > 10 * one


def test_dump_outputs_samples_at_fixed_positions_under_the_size_cap(tmp_path, monkeypatch):
    import numpy as np
    import torch
    monkeypatch.setattr(bench, "DUMP_ELEMS_PER_ARRAY", 3000)
    g = torch.Generator().manual_seed(0)
    params = [torch.randn(50, 40, generator=g), torch.randn(7, generator=g), torch.randn(300, generator=g)]
    opt = types.SimpleNamespace(state={params[0]: {"exp_avg": params[0] * 2, "exp_avg_sq": params[0] ** 2},
                                       params[2]: {"exp_avg": params[2] * 2, "exp_avg_sq": params[2] ** 2}},
                                last_grad_norm=torch.tensor(0.25))
    bench.dump_outputs(str(tmp_path / "a"), params, opt, 1.5)
    bench.dump_outputs(str(tmp_path / "b"), params, opt, 1.5)
    a = {f.stem: np.load(f) for f in (tmp_path / "a").glob("*.npy")}
    b = {f.stem: np.load(f) for f in (tmp_path / "b").glob("*.npy")}
    assert set(a) == {"loss", "params", "adam_exp_avg", "adam_exp_avg_sq", "grad_norm"}
    assert a["loss"].dtype == np.float64 and float(a["loss"][0]) == 1.5 and float(a["grad_norm"][0]) == 0.25
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    # share 1000 per tensor: 1000 sampled of the 2000-element tensor, the small ones whole
    assert a["params"].shape == (1000 + 7 + 300,)
    assert np.array_equal(a["params"][1000:1007], params[1].numpy()) and np.array_equal(a["params"][1007:], params[2].numpy())
    assert np.isin(a["params"][:1000], params[0].numpy()).all()
    want = np.concatenate([2 * a["params"][:1000], np.zeros(7, np.float32), 2 * a["params"][1007:]])
    np.testing.assert_array_equal(a["adam_exp_avg"], want)           # same positions; no optimizer state: zero moments
    assert not a["adam_exp_avg_sq"][1000:1007].any()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_steps_below_one_is_refused_before_any_device_work():
    import subprocess
    import sys
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(bench.__file__), "bench.py"), "--steps", "0"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 2 and "--steps" in p.stderr, p.stderr[-1000:]
