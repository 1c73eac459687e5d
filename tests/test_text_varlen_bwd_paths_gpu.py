"""The three backward entries of the packed (variable-length) text tower through the C ABI: the causal
attention backward inside packed sequences, the token / position scatter of the embedding and the transpose of the first-EOS
gather.  After tests/test_text_varlen_paths_gpu.py: outputs live in guarded buffers pre-filled with NaN, the rows behind every
operand are NaN, a refused call launches nothing and writes nothing.  References: fp64 attention with a causal mask per sequence
(tests/kernel_checks.py, the project's tolerances), index expressions on the host for the two scatters."""
import pytest
import torch

from tests import kernel_checks as kc
from tests import schedule_checks as sc
from tests.test_varlen_paths_gpu import HD, cumulative, i32, ok, stream, unwritten

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from dclip_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------------------------------------ causal attention backward

ATTN_CASES = [([1, 2, 17, 63, 64, 65, 77, 5], 2), ([128, 129, 3], 1), ([64], 3)]
SITE = "attention_varlen_causal_bwd"


def run_backward(lib, dev, qkv, dout, lengths, H):
    """dqkv [Tp, 3*H*64] of one forward (out / lse made on the device by dclip_attention_varlen_causal_fwd) and one backward."""
    N, T, D = len(lengths), sum(lengths), H * HD
    src, dsrc = kc.poisoned(qkv, 3 * D, dev), kc.poisoned(dout, D, dev)
    out = kc.poisoned(torch.zeros((T, D)), D, dev)                      # [T] rows are overwritten, NaN rows stay behind them
    lse, delta = kc.Guarded(H, T, device=dev), kc.Guarded(H, T, device=dev)
    cu = i32(cumulative(lengths), dev)
    assert lib.dclip_attention_varlen_causal_fwd(src.data_ptr(), cu.data_ptr(), out.data_ptr(), lse.ptr, N, max(lengths), H, 0,
                                                 stream()) == 0, lib.dclip_last_error()
    dqkv = kc.Guarded(T, 3 * D, device=dev)
    ok(lib, lib.dclip_attention_varlen_causal_bwd(src.data_ptr(), cu.data_ptr(), out.data_ptr(), dsrc.data_ptr(), lse.ptr, dqkv.ptr,
                                                  delta.ptr, N, max(lengths), H, stream()), SITE)
    torch.cuda.synchronize()
    dqkv.assert_guards(SITE + " dqkv")
    delta.assert_guards(SITE + " delta")
    lse.assert_guards(SITE + " lse")
    return dqkv.get()


def per_sequence(dqkv, lengths, H):
    """[(dq, dk, dv)] per sequence, each [S, H*64]."""
    cu, D = cumulative(lengths), H * HD
    return [tuple(dqkv[cu[n]:cu[n + 1], i * D:(i + 1) * D] for i in range(3)) for n in range(len(lengths))]


def backward_reference(qkv, dout, lengths, H):
    cu, ref = cumulative(lengths), []
    for n, S in enumerate(lengths):
        q, k, v = (qkv[cu[n]:cu[n + 1]].double().view(1, S, 3, H, HD)[:, :, i] for i in range(3))
        do = dout[cu[n]:cu[n + 1]].double().view(1, S, H, HD)
        _, _, dq, dk, dv = kc.attention_math(q, k, v, do, kc._causal_mask(S, torch.float64, "cpu"))
        ref.append(tuple(t.reshape(S, H * HD) for t in (dq, dk, dv)))
    return ref


def bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("lengths,H", ATTN_CASES, ids=["tile_edges", "128_129_3", "one_full_tile"])
def test_causal_varlen_backward_against_fp64_per_sequence(dev, lib, lengths, H):
    """dq / dk / dv per sequence at kc.TOL_ATTN_BWD; a one-row sequence's dq and dk have an identically zero reference, where
    check_blocks demands exact zeros; every word of dqkv is written (finite); a second run gives the same bits.
    Measured on an MI355X, worst block per case: dq 1.08e-6 / 8.6e-7 / 5.3e-7, dk 1.47e-6 / 1.08e-6 / 6.5e-7, dv 4.9e-7 / 6.3e-7 /
    4.3e-7 (gate 5e-5)."""
    T, D = sum(lengths), H * HD
    qkv, dout = kc._gauss((T, 3 * D), 51, 1.5), kc._gauss((T, D), 52, 1.5)
    dqkv = run_backward(lib, dev, qkv, dout, lengths, H)
    assert bool(torch.isfinite(dqkv).all()), f"{int((~torch.isfinite(dqkv)).sum())} words of dqkv were not written"
    got, want = per_sequence(dqkv, lengths, H), backward_reference(qkv, dout, lengths, H)
    blocks = {}
    for n, (g, w) in enumerate(zip(got, want)):
        for name, a, b in zip(("dq", "dk", "dv"), g, w):
            blocks[f"{name}[{n}:S={lengths[n]}]"] = (a, b, kc.TOL_ATTN_BWD)
    fig = kc.check_blocks(blocks, f"{SITE} {lengths} H={H}")
    print({name: max(v for k, v in fig.items() if k.startswith(name)) for name in ("dq", "dk", "dv")})
    cu = cumulative(lengths)
    for n, S in enumerate(lengths):
        if S == 1:                                                       # dv = dout itself, bit for bit
            assert bits_equal(got[n][2], dout[cu[n]:cu[n + 1]])
    assert bits_equal(run_backward(lib, dev, qkv, dout, lengths, H), dqkv), "two runs differ"


@pytest.mark.parametrize("lengths,H,victim", [(ATTN_CASES[0][0], 2, 4), (ATTN_CASES[1][0], 1, 1)], ids=["tile_edges", "128_129_3"])
def test_a_nan_sequence_leaves_every_other_sequence_bit_identical(dev, lib, lengths, H, victim):
    T, D = sum(lengths), H * HD
    qkv, dout = kc._gauss((T, 3 * D), 53, 1.5), kc._gauss((T, D), 54, 1.5)
    clean = per_sequence(run_backward(lib, dev, qkv, dout, lengths, H), lengths, H)
    cu = cumulative(lengths)
    bad_qkv, bad_dout = qkv.clone(), dout.clone()
    bad_qkv[cu[victim]:cu[victim + 1]] = kc.NAN
    bad_dout[cu[victim]:cu[victim + 1]] = kc.NAN
    dirty = per_sequence(run_backward(lib, dev, bad_qkv, bad_dout, lengths, H), lengths, H)
    for n in range(len(lengths)):
        if n == victim:
            assert all(bool(torch.isnan(t).all()) for t in dirty[n])
            continue
        for a, b, name in zip(clean[n], dirty[n], ("dq", "dk", "dv")):
            assert bool(torch.isfinite(b).all()), (n, name)
            assert bits_equal(a, b), f"sequence {n} {name} changed with sequence {victim}"


def test_later_rows_change_no_earlier_query_gradient(dev, lib):
    """A 65-row sequence between two others.  dout of rows 64.. set to 1e4: rows 64.. attend to keys 0..63, so dk / dv of those
    keys change, while dq of rows 0..63 (which depends on their own dout only) stays bit-equal.  k of rows 64.. set to 1e4: under
    the causal mask rows 0..63 see none of them — across the tile edge — and their dq stays bit-equal.  The neighbours never
    change."""
    lengths, H = [5, 65, 9], 2
    T, D = sum(lengths), H * HD
    qkv, dout = kc._gauss((T, 3 * D), 55, 1.5), kc._gauss((T, D), 56, 1.5)
    cu = cumulative(lengths)
    clean = per_sequence(run_backward(lib, dev, qkv, dout, lengths, H), lengths, H)
    big_dout = dout.clone()
    big_dout[cu[1] + 64:cu[2]] = 1e4
    a = per_sequence(run_backward(lib, dev, qkv, big_dout, lengths, H), lengths, H)
    assert bits_equal(clean[1][0][:64], a[1][0][:64]), "dq of rows 0..63 changed with dout of row 64"
    assert not torch.equal(clean[1][1][:64], a[1][1][:64]) and not torch.equal(clean[1][2][:64], a[1][2][:64])
    assert all(bool(torch.isfinite(t).all()) for t in a[1])
    big_k = qkv.clone()
    big_k[cu[1] + 64:cu[2], D:2 * D] = 1e4
    b = per_sequence(run_backward(lib, dev, big_k, dout, lengths, H), lengths, H)
    assert bits_equal(clean[1][0][:64], b[1][0][:64]), "dq of rows 0..63 changed with k of row 64"
    assert all(bool(torch.isfinite(t).all()) for t in b[1])
    for other in (a, b):
        for n in (0, 2):
            assert all(bits_equal(x, y) for x, y in zip(clean[n], other[n])), n


# ------------------------------------------------------------------------------------------------ embedding backward

def embed_case(D):
    lens, T, vocab = [1, 16, 3, 9], 16, 50
    g = torch.Generator().manual_seed(D)
    ids = torch.full((len(lens), T), 2 ** 40, dtype=torch.int64)          # pad ids far outside the table: never read
    ids[1, 10:] = -(2 ** 40)
    for n, L in enumerate(lens):
        ids[n, :L] = torch.randint(0, vocab, (L,), generator=g)
    ids[1, 0], ids[1, 1], ids[3, 2] = vocab + 7, -3, vocab - 1              # inside a caption the id clamp applies
    ids[1, 5] = ids[1, 4]                                                   # a repeated id inside one caption ...
    ids[3, 1], ids[2, 1] = ids[1, 4], ids[1, 4]                             # ... and across captions
    dx = kc._gauss((sum(lens), D), 61)
    return lens, T, vocab, ids, dx


@pytest.mark.parametrize("D", [8, 512])
def test_text_embed_varlen_bwd_against_the_host_scatter(dev, lib, D):
    lens, T, vocab, ids, dx = embed_case(D)
    cu = cumulative(lens)
    want_pos = torch.zeros((T, D))
    for n, L in enumerate(lens):                                            # ascending caption order, fp32: the kernel's sum
        want_pos[:L] += dx[cu[n]:cu[n + 1]]
    packed_ids = torch.cat([ids[n, :L].clamp(0, vocab - 1) for n, L in enumerate(lens)])
    want_tok = torch.zeros((vocab, D), dtype=torch.float64).index_add_(0, packed_ids, dx.double())
    bound = sc.embed_atomic_bound(packed_ids, dx, vocab)
    d_ids, d_cu, d_dx = ids.to(dev), i32(cu, dev), kc.poisoned(dx, D, dev)
    site = "text_embed_varlen_bwd"

    def call(want_tok_out, want_pos_out):
        dtok = kc.Guarded(vocab, D, device=dev, fill=0.0)
        dpos = kc.Guarded(T + 4, D, device=dev)                             # four rows behind T: untouched
        ok(lib, lib.dclip_text_embed_varlen_bwd(d_ids.data_ptr(), d_cu.data_ptr(), d_dx.data_ptr(), dtok.ptr if want_tok_out else None,
                                                dpos.ptr if want_pos_out else None, len(lens), T, D, vocab, stream()), site)
        torch.cuda.synchronize()
        dtok.assert_guards(site + " dtok")
        dpos.assert_guards(site + " dpos")
        return dtok, dpos

    dtok, dpos = call(True, True)
    assert torch.equal(dpos.get()[:T], want_pos), "dpos is not the sum in ascending caption order"
    assert float(want_pos[9:].abs().max()) > 0 and bool((want_pos[T - 1] == dx[cu[1] + T - 1]).all())
    assert bool(unwritten(dpos)[T:].all()), "rows >= T of dpos were written"
    diff = (dtok.get().double() - want_tok).abs()
    assert bool((diff <= bound).all()), float((diff - bound).max())
    tok_only, pos_none = call(True, False)
    assert bool(unwritten(pos_none).all()), "dpos = NULL, yet the dpos buffer was written"
    assert bool(((tok_only.get().double() - want_tok).abs() <= bound).all())
    tok_none, pos_only = call(False, True)
    assert torch.equal(tok_none.get(), torch.zeros((vocab, D))), "dtok = NULL, yet the dtok buffer was written"
    assert bits_equal(pos_only.get()[:T], dpos.get()[:T])
    # a caption that stops before the longest: its position rows hold zeros where no caption reaches
    short_cu = i32(cumulative([1, 5, 3, 2]), dev)
    dp = kc.Guarded(T, D, device=dev)
    ok(lib, lib.dclip_text_embed_varlen_bwd(d_ids.data_ptr(), short_cu.data_ptr(), d_dx.data_ptr(), None, dp.ptr, len(lens), T, D,
                                            vocab, stream()), site)
    torch.cuda.synchronize()
    assert torch.equal(dp.get()[5:], torch.zeros((T - 5, D))) and float(dp.get()[4].abs().max()) > 0


@pytest.mark.parametrize("D", [8, 512])
def test_scatter_last_rows_equals_the_host_expression(dev, lib, D):
    lens = [1, 2, 3, 12]
    cu = cumulative(lens)
    dout = kc._gauss((len(lens), D), 71)
    want = torch.zeros((sum(lens), D))
    for n in range(len(lens)):
        want[cu[n + 1] - 1] = dout[n]
    dx = kc.Guarded(sum(lens), D, device=dev)
    d_dout, d_cu = kc.poisoned(dout, D, dev), i32(cu, dev)
    ok(lib, lib.dclip_scatter_last_rows(d_dout.data_ptr(), d_cu.data_ptr(), dx.ptr, len(lens), D, stream()), "scatter_last_rows")
    torch.cuda.synchronize()
    dx.assert_guards("scatter_last_rows")
    assert not bool(unwritten(dx).any()), "a word of dx was not written"
    assert torch.equal(dx.get(), want)


# ------------------------------------------------------------------------------------------------ refusals

def test_refusals_launch_nothing_and_write_nothing(dev, lib):
    H, D, N, T = 2, 8, 2, 7
    W = H * HD
    f = kc.poisoned(kc._gauss((T, 3 * W), 1), 3 * W, dev)
    tab = i32([0, 3, 7, 0, 0, 0, 0, 0], dev)                     # stands in for the int32 table; a refusal never reads it
    ids = torch.zeros((N, T), dtype=torch.int64, device=dev)
    outs = {k: kc.Guarded(T, 3 * W, device=dev) for k in ("dqkv", "delta", "dtok", "dpos", "dx")}
    lib.dclip_relu_f32(kc.Guarded(1, 64, device=dev).ptr, 64, stream())               # some other launch site
    s = stream()
    fp = f.data_ptr()
    calls = {
        "attn": (lib.dclip_attention_varlen_causal_bwd,
                 [fp, tab.data_ptr(), fp, fp, fp, outs["dqkv"].ptr, outs["delta"].ptr, N, 4, H, s],
                 [(0, None), (1, None), (2, None), (3, None), (4, None), (5, None), (6, None), (7, 0), (7, -1), (8, 0), (9, 0), (9, -2),
                  (0, fp + 4), (2, fp + 8), (3, fp + 4), (5, outs["dqkv"].ptr + 8), (1, tab.data_ptr() + 2), (4, fp + 2),
                  (6, outs["delta"].ptr + 2)]),
        "embed": (lib.dclip_text_embed_varlen_bwd,
                  [ids.data_ptr(), tab.data_ptr(), fp, outs["dtok"].ptr, outs["dpos"].ptr, N, T, D, 10, s],
                  [(0, None), (1, None), (2, None), (5, 0), (5, -1), (6, 0), (7, 0), (7, 6), (7, -4), (8, 0), (2, fp + 4),
                   (4, outs["dpos"].ptr + 8), (3, outs["dtok"].ptr + 2), (0, ids.data_ptr() + 4), (1, tab.data_ptr() + 2)]),
        "scatter": (lib.dclip_scatter_last_rows, [fp, tab.data_ptr(), outs["dx"].ptr, N, D, s],
                    [(0, None), (1, None), (2, None), (3, 0), (3, -3), (4, 0), (4, 6), (4, -4), (0, fp + 4), (2, outs["dx"].ptr + 8),
                     (1, tab.data_ptr() + 2)]),
    }
    for name, (fn, good, bad) in calls.items():
        for at, value in bad:
            args = list(good)
            args[at] = value
            assert fn(*args) == kc.E_INVAL, (name, at, value)
            assert lib.dclip_last_error()
            assert lib.dclip_last_launch() == b"relu_f32", f"a refused {name} call launched"
    both_null = list(calls["embed"][1])
    both_null[3] = both_null[4] = None                           # dtok and dpos both NULL
    assert lib.dclip_text_embed_varlen_bwd(*both_null) == kc.E_INVAL and lib.dclip_last_launch() == b"relu_f32"
    torch.cuda.synchronize()
    for name, t in outs.items():
        t.assert_guards(f"refused {name}")
        assert bool(unwritten(t).all()), f"a refused {name} call wrote"
