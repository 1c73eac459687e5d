"""CPU-only: the grid plumbing around the two new ops, with the fp64 reference of tests/kernel_checks_interp.py standing in
for them (no kernel runs here): which grid get_image_features takes from the pixels, what the engine hands to
pos_interp_fwd, and where the position gradient of another grid is written."""
import numpy as np
import pytest
import torch

from dclip_amd import config as dcfg, engine, ops
from dclip_amd.clip_model import HipCLIPModel
from tests import kernel_checks_interp as ki


def pos_interp_fwd(pos, g, gh, gw):
    return torch.from_numpy(ki.interp_reference(pos.numpy(), g, gh, gw).astype(np.float32))


def pos_interp_bwd(dout, g, gh, gw, out=None, accumulate=False):
    assert out is not None and not accumulate
    out.copy_(torch.from_numpy(ki.interp_bwd_reference(dout.numpy(), g, gh, gw).astype(np.float32)))
    return out


@pytest.fixture()
def reference_ops(monkeypatch):
    monkeypatch.setattr(ops, "pos_interp_fwd", pos_interp_fwd)
    monkeypatch.setattr(ops, "pos_interp_bwd", pos_interp_bwd)


def test_the_grid_comes_from_the_pixels_and_the_size_check_stays():
    m = HipCLIPModel(dcfg.tiny())                         # 64 px, patch 16
    z = lambda h, w: torch.zeros(1, 3, h, w)              # noqa: E731
    assert m._vision_grid(z(64, 64), False) is None and m._vision_grid(z(64, 64), True) is None
    assert m._vision_grid(z(96, 96), True) == (6, 6)
    assert m._vision_grid(z(64, 112), True) == (4, 7)     # (rows, columns)
    assert m._vision_grid(z(80, 50), True) == (5, 3)      # floor: trailing rows and columns belong to no patch
    assert m._vision_grid(z(70, 70), True) == (4, 4)
    for kw in ({}, {"interpolate_pos_encoding": False}):
        with pytest.raises(ValueError, match="doesn't match model"):
            m.get_image_features(pixel_values=z(96, 96), **kw)
    with pytest.raises(ValueError, match="smaller than one patch"):
        m.get_image_features(pixel_values=z(64, 10), interpolate_pos_encoding=True)


def test_engine_resamples_the_table_and_transposes_its_gradient_into_the_allocated_slice(reference_ops):
    v = dcfg.tiny().vision
    g, D = v.grid, v.hidden_size
    rng = np.random.default_rng(0)
    pos = torch.from_numpy(rng.standard_normal((1 + g * g, D)).astype(np.float32))
    p = engine.VisionParams(None, None, pos, None, None, [], None, None, None)
    assert engine._grid_seq(v, None) == v.seq_len and engine._grid_seq(v, (4, 7)) == 29
    table = engine._grid_front(p, torch.zeros(2, 3, 64, 112), v, (4, 7))
    assert table.shape == (29, D) and torch.equal(table[0], pos[0])
    assert np.array_equal(table.numpy(), ki.interp_reference(pos.numpy(), g, 4, 7).astype(np.float32))
    with pytest.raises(ValueError, match="do not make a 7x4 grid"):
        engine._grid_front(p, torch.zeros(2, 3, 64, 112), v, (7, 4))
    # backward: the [S*D] column sum goes through the transpose into the parameter's own [1 + g*g, D] slice
    colsum = torch.from_numpy(rng.standard_normal(29 * D).astype(np.float32))
    bucket = torch.full((3 + (1 + g * g) * D,), float("nan"))
    asked = []

    def alloc(name, shape):
        asked.append((name, tuple(shape)))
        return bucket[3:].view(shape)

    grad = engine._grid_pos_grad(colsum, p, v, (4, 7), alloc, torch.device("cpu"))
    assert asked == [("pos", (1 + g * g, D))] and grad.shape == pos.shape and grad.data_ptr() == bucket[3:].data_ptr()
    want = ki.interp_bwd_reference(colsum.view(29, D).numpy(), g, 4, 7)
    assert np.array_equal(grad.numpy(), want.astype(np.float32)) and bool(torch.isnan(bucket[:3]).all())
    # <backward(dout), pos> == <dout, forward(pos)>
    lhs, rhs = float((grad.double() * pos.double()).sum()), float((colsum.view(29, D).double() * table.double()).sum())
    assert abs(lhs - rhs) <= 1e-4 * max(1.0, abs(rhs))
