"""The three entries of the packed (variable-length) text tower through the C ABI: the token / position
gather on captions cut after their first EOS, causal self-attention inside packed sequences and the word-token packing on
packed rows.  After tests/test_varlen_paths_gpu.py: outputs live in guarded buffers, the rows behind every operand are NaN, a
refused call launches nothing and writes nothing.  References: fp64 attention with a causal mask (tests/kernel_checks.py, the
project's tolerances), an index expression on the host for the gather, ops.pack_tokens on the padded counterpart."""
import pytest
import torch

from tests import kernel_checks as kc
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


# ------------------------------------------------------------------------------------------------ causal attention

ATTN_CASES = [([1, 2, 17, 63, 64, 65, 77, 5], 2), ([128, 129, 3], 1), ([64], 3)]
SITE = "attention_varlen_causal_fwd"


def run_attention(lib, dev, qkv, lengths, H, last_only, with_lse=True):
    """(out [rows, H*64], lse [H, rows] or None) of one call; rows = Tp, or N with last_only."""
    N, T, D = len(lengths), sum(lengths), H * HD
    src = kc.poisoned(qkv, 3 * D, dev)                                 # NaN rows behind the last sequence
    rows = N if last_only else T
    out, lse = kc.Guarded(rows, D, device=dev), kc.Guarded(H, rows, device=dev)
    cu = i32(cumulative(lengths), dev)
    ok(lib, lib.dclip_attention_varlen_causal_fwd(src.data_ptr(), cu.data_ptr(), out.ptr, lse.ptr if with_lse else None, N,
                                                  max(lengths), H, int(last_only), stream()), SITE)
    torch.cuda.synchronize()
    out.assert_guards(SITE + " out")
    lse.assert_guards(SITE + " lse")
    if not with_lse:
        assert bool(unwritten(lse).all()), "lse = NULL, yet the lse buffer was written"
    return out.get(), lse.get() if with_lse else None


def attention_reference(qkv, lengths, H, last_only):
    """Per sequence (out_n, lse_n [H, rows_n]) in fp64: causal, or the last row over all keys."""
    cu, ref = cumulative(lengths), []
    for n, S in enumerate(lengths):
        q, k, v = (qkv[cu[n]:cu[n + 1]].double().view(1, S, 3, H, HD)[:, :, i] for i in range(3))
        if last_only:
            out, lse, _, _, _ = kc.attention_math(q[:, S - 1:], k, v, None)
        else:
            out, lse, _, _, _ = kc.attention_math(q, k, v, None, kc._causal_mask(S, torch.float64, "cpu"))
        ref.append((out.reshape(-1, H * HD), lse.reshape(H, -1)))
    return ref


def per_sequence(out, lse, lengths, last_only):
    cu = list(range(len(lengths) + 1)) if last_only else cumulative(lengths)
    return [(out[cu[n]:cu[n + 1]], None if lse is None else lse[:, cu[n]:cu[n + 1]]) for n in range(len(lengths))]


@pytest.mark.parametrize("last_only", [False, True], ids=["all_rows", "last_only"])
@pytest.mark.parametrize("lengths,H", ATTN_CASES, ids=["tile_edges", "128_129_3", "one_full_tile"])
def test_causal_varlen_attention_against_fp64_per_sequence(dev, lib, lengths, H, last_only):
    qkv = kc._gauss((sum(lengths), 3 * H * HD), 21, 1.5)
    out, lse = run_attention(lib, dev, qkv, lengths, H, last_only)
    got, want = per_sequence(out, lse, lengths, last_only), attention_reference(qkv, lengths, H, last_only)
    blocks = {}
    for n, ((o, l), (wo, wl)) in enumerate(zip(got, want)):
        blocks[f"out[{n}:S={lengths[n]}]"] = (o, wo, kc.TOL_ATTN_FWD)
        blocks[f"lse[{n}:S={lengths[n]}]"] = (l, wl, kc.TOL_LSE)
    fig = kc.check_blocks(blocks, f"{SITE} {lengths} H={H} last_only={last_only}")
    print("worst out", max(v for k, v in fig.items() if k.startswith("out")), "worst lse",
          max(v for k, v in fig.items() if k.startswith("lse")))
    out2, _ = run_attention(lib, dev, qkv, lengths, H, last_only, with_lse=False)
    assert torch.equal(out2.view(torch.int32), out.view(torch.int32)), "lse = NULL changed out"


@pytest.mark.parametrize("last_only", [False, True], ids=["all_rows", "last_only"])
@pytest.mark.parametrize("lengths,H,victim", [(ATTN_CASES[0][0], 2, 4), (ATTN_CASES[1][0], 1, 1)], ids=["tile_edges", "128_129_3"])
def test_a_nan_sequence_leaves_every_other_sequence_bit_identical(dev, lib, lengths, H, victim, last_only):
    qkv = kc._gauss((sum(lengths), 3 * H * HD), 22, 1.5)
    clean = per_sequence(*run_attention(lib, dev, qkv, lengths, H, last_only), lengths, last_only)
    cu = cumulative(lengths)
    dirty_in = qkv.clone()
    dirty_in[cu[victim]:cu[victim + 1]] = kc.NAN
    dirty = per_sequence(*run_attention(lib, dev, dirty_in, lengths, H, last_only), lengths, last_only)
    for n in range(len(lengths)):
        if n == victim:
            assert bool(torch.isnan(dirty[n][0]).all())
            continue
        for a, b, name in zip(clean[n], dirty[n], ("out", "lse")):
            assert bool(torch.isfinite(b).all()), (n, name)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"sequence {n} {name} changed with sequence {victim}"


def test_huge_later_keys_change_no_earlier_row(dev, lib):
    """A 65-row sequence between two others: k of rows 64.. set to 1e4 (finite).  Under the causal mask rows 0..63 see none of
    them — inside the first key tile (row 63 against key 64 would be the next tile) and across tiles — so they stay bit-equal;
    row 64 changes."""
    lengths, H = [5, 65, 9], 2
    D = H * HD
    qkv = kc._gauss((sum(lengths), 3 * D), 23, 1.5)
    clean = per_sequence(*run_attention(lib, dev, qkv, lengths, H, False), lengths, False)
    cu = cumulative(lengths)
    huge = qkv.clone()
    huge[cu[1] + 64:cu[2], D:2 * D] = 1e4
    after = per_sequence(*run_attention(lib, dev, huge, lengths, H, False), lengths, False)
    for n in (0, 2):
        for a, b in zip(clean[n], after[n]):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), n
    for a, b in zip(clean[1], after[1]):
        assert bool(torch.isfinite(b).all())
    assert torch.equal(clean[1][0][:64].view(torch.int32), after[1][0][:64].view(torch.int32))
    assert torch.equal(clean[1][1][:, :64].view(torch.int32), after[1][1][:, :64].view(torch.int32))
    assert not torch.equal(clean[1][0][64], after[1][0][64])


# ------------------------------------------------------------------------------------------------ embedding gather

@pytest.mark.parametrize("D", [8, 512])
def test_text_embed_varlen_equals_the_host_gather_and_never_reads_the_pads(dev, lib, D):
    lens, T, vocab = [1, 16, 3, 9], 16, 50
    g = torch.Generator().manual_seed(D)
    ids = torch.full((len(lens), T), 2 ** 40, dtype=torch.int64)          # pad ids far outside the table: never read
    ids[1, 10:] = -(2 ** 40)
    for n, L in enumerate(lens):
        ids[n, :L] = torch.randint(0, vocab, (L,), generator=g)
    ids[1, 0], ids[1, 1], ids[3, 2] = vocab + 7, -3, vocab - 1              # inside a caption the id clamp applies
    tok, pos = kc._gauss((vocab, D), 31), kc._gauss((T + 4, D), 32)
    want = torch.cat([tok[ids[n, :L].clamp(0, vocab - 1)] + pos[:L] for n, L in enumerate(lens)])
    d_tok, d_pos = kc.poisoned(tok, D, dev), kc.poisoned(pos, D, dev)
    x = kc.Guarded(sum(lens), D, device=dev)
    cu = i32(cumulative(lens), dev)
    d_ids = ids.to(dev)
    ok(lib, lib.dclip_text_embed_varlen(d_ids.data_ptr(), cu.data_ptr(), d_tok.data_ptr(), d_pos.data_ptr(), x.ptr, len(lens), T, D,
                                        vocab, stream()), "text_embed_varlen")
    torch.cuda.synchronize()
    x.assert_guards("text_embed_varlen x")
    assert torch.equal(x.get(), want)
    # the padded entry on the same captions, row by row (its pads clamped): the same statement, the same bits
    full = torch.empty((len(lens) * T, D), dtype=torch.float32, device=dev)
    assert lib.dclip_text_embed_fwd(d_ids.data_ptr(), d_tok.data_ptr(), d_pos.data_ptr(), full.data_ptr(), len(lens), T, D, vocab,
                                    stream()) == 0
    torch.cuda.synchronize()
    padded = torch.cat([full.cpu().view(len(lens), T, D)[n, :L] for n, L in enumerate(lens)])
    assert torch.equal(x.get().view(torch.int32), padded.view(torch.int32))


# ------------------------------------------------------------------------------------------------ token packing

@pytest.mark.parametrize("Tmax", [1, 10])
def test_pack_tokens_varlen_equals_pack_tokens_on_the_padded_counterpart(dev, lib, Tmax):
    from dclip_amd import ops
    lens, T, Pd = [1, 2, 3, 12], 12, 8                 # word tokens: 0 (no EOS / EOS at 0), 0, 1, 10
    tokens = kc._gauss((sum(lens), Pd), 41)
    sentence = kc._gauss((len(lens), Pd), 42)
    cu = cumulative(lens)
    padded = kc._gauss((len(lens), T, Pd), 43)         # the pad rows hold other values: neither form may read them
    for n, L in enumerate(lens):
        padded[n, :L] = tokens[cu[n]:cu[n + 1]]
    eos = i32([L - 1 for L in lens], dev)
    want = ops.pack_tokens(padded.to(dev).contiguous(), sentence.to(dev).contiguous(), eos, Tmax).cpu()
    out = kc.Guarded(len(lens) * Tmax, Pd, device=dev)
    d_tok, d_sent = kc.poisoned(tokens, Pd, dev), kc.poisoned(sentence, Pd, dev)
    d_cu = i32(cu, dev)
    ok(lib, lib.dclip_pack_tokens_varlen(d_tok.data_ptr(), d_sent.data_ptr(), d_cu.data_ptr(), out.ptr, len(lens), Tmax, Pd,
                                         stream()), "pack_tokens_varlen")
    torch.cuda.synchronize()
    out.assert_guards("pack_tokens_varlen")
    got = out.get().view(len(lens), Tmax, Pd)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(got[0, 0], sentence[0]) and torch.equal(got[1, 0], sentence[1]) and torch.equal(got[2, 0], tokens[cu[2] + 1])
    if Tmax > 1:
        assert float(got[2, 1:].abs().max()) == 0.0 and float(got[0, 1:].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ refusals

def test_refusals_launch_nothing_and_write_nothing(dev, lib):
    H, D, N, T = 2, 8, 2, 7
    f = kc.poisoned(kc._gauss((T, 3 * H * HD), 1), 3 * H * HD, dev)
    tab = i32([0, 3, 7, 0, 0, 0, 0, 0], dev)                     # stands in for the int32 table; a refusal never reads it
    ids = torch.zeros((N, T), dtype=torch.int64, device=dev)
    outs = {k: kc.Guarded(T, H * HD, device=dev) for k in ("attn", "lse", "x", "pack")}
    lib.dclip_relu_f32(kc.Guarded(1, 64, device=dev).ptr, 64, stream())               # some other launch site
    s = stream()
    calls = {
        "attn": (lib.dclip_attention_varlen_causal_fwd,
                 [f.data_ptr(), tab.data_ptr(), outs["attn"].ptr, outs["lse"].ptr, N, 4, H, 0, s],
                 [(0, None), (1, None), (2, None), (4, 0), (4, -1), (5, 0), (6, 0), (6, -2), (0, f.data_ptr() + 4),
                  (2, outs["attn"].ptr + 8), (1, tab.data_ptr() + 2), (3, outs["lse"].ptr + 2)]),
        "x": (lib.dclip_text_embed_varlen, [ids.data_ptr(), tab.data_ptr(), f.data_ptr(), f.data_ptr(), outs["x"].ptr, N, T, D, 10, s],
              [(0, None), (1, None), (2, None), (3, None), (4, None), (5, 0), (5, -1), (6, 0), (7, 0), (7, 6), (7, -4), (8, 0),
               (2, f.data_ptr() + 4), (3, f.data_ptr() + 8), (4, outs["x"].ptr + 8), (0, ids.data_ptr() + 4), (1, tab.data_ptr() + 2)]),
        "pack": (lib.dclip_pack_tokens_varlen, [f.data_ptr(), f.data_ptr(), tab.data_ptr(), outs["pack"].ptr, N, 2, D, s],
                 [(0, None), (1, None), (2, None), (3, None), (4, 0), (4, -3), (5, 0), (6, 0), (6, 6), (0, f.data_ptr() + 4),
                  (1, f.data_ptr() + 8), (3, outs["pack"].ptr + 4), (2, tab.data_ptr() + 2)]),
    }
    for name, (fn, good, bad) in calls.items():
        for at, value in bad:
            args = list(good)
            args[at] = value
            assert fn(*args) == kc.E_INVAL, (name, at, value)
            assert lib.dclip_last_error()
            assert lib.dclip_last_launch() == b"relu_f32", f"a refused {name} call launched"
    torch.cuda.synchronize()
    for name, t in outs.items():
        t.assert_guards(f"refused {name}")
        assert bool(unwritten(t).all()), f"a refused {name} call wrote"
