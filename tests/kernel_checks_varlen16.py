"""Checks for the 16-bit packed attention core (dclip_amd/csrc/attention_varlen16.hip): packs of sequences of
different lengths built from the per-sequence data of tests/kernel_checks.py (exact selection, Gaussian), the exact and the
bounded check per sequence, a fp64 emulation of the two kernels' documented roundings, and the C ABI call on guarded buffers.
Nothing above `run_pack` touches the product or the GPU."""
from types import SimpleNamespace

import torch

from tests.kernel_checks import (HD, MIN_MARGIN, NAN16, TYPES16, Attn16Case, Guarded, attn16_forward, attn16_out_bound, poisoned,
                                 round16, selection_data)

MODES = ("full", "causal", "cls", "last")          # tiled non-causal / tiled causal / row entry last = 0 / row entry last = 1
SITES = {"full": "attention_varlen_fwd_%s", "causal": "attention_varlen_fwd_%s", "cls": "attention_varlen_row_fwd_%s",
         "last": "attention_varlen_row_fwd_%s"}


def cumulative(lengths):
    cu = [0]
    for S in lengths:
        cu.append(cu[-1] + S)
    return cu


def _rows(t):                          # [1][H][S][64] -> [S][H*64]
    _, H, S, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(S, H * HD)


def build_pack(lengths, H, ty: str, mode: str, data: str, seed: int = 0):
    """N sequences, sequence n = the data of kernel_checks for (B = 1, S_n, H): `select` (exact selection; the row entry's
    query sees every key, so its data are the non-causal ones) or `gauss` (scale 1.5, rounded to the type).  A length of 0
    gives an empty sequence (None).  pack.qkv [T][3*H*64] fp64 holds values exact in the type."""
    assert mode in MODES and data in ("select", "gauss")
    t16 = TYPES16[ty]
    row = mode in ("cls", "last")
    seqs, blocks = [], []
    for n, S in enumerate(lengths):
        if S == 0:
            seqs.append(None)
            continue
        case = Attn16Case("row" if row else "fwd", ty, 1, S, H, mode == "causal", (S - 1,) if mode == "last" else None)
        s = SimpleNamespace(case=case, ty=t16, data=data, rows=torch.tensor([S - 1], dtype=torch.int32) if mode == "last" else None)
        if data == "select":
            s.q, s.k, s.v, _, s.pi, s.margin = selection_data(1, S, H, mode == "causal", 7919 * seed + 131 * n + 31 * S + 2 * H)
        else:
            g = torch.Generator().manual_seed(1000 * seed + 100 + 17 * n + S)
            s.q, s.k, s.v = ((torch.randn((1, H, S, HD), generator=g) * 1.5).to(t16.dtype).double() for _ in range(3))
        seqs.append(s)
        blocks.append(torch.cat([_rows(s.q), _rows(s.k), _rows(s.v)], 1))
    return SimpleNamespace(lengths=list(lengths), H=H, ty=t16, tyname=ty, mode=mode, row=row, data=data, seqs=seqs,
                           qkv=torch.cat(blocks), cu=cumulative(lengths))


def out_rows(pack) -> int:
    return len(pack.lengths) if pack.row else pack.cu[-1]


def per_sequence(pack, out):
    """out [T][D] (tiled) or [N][D] (row entry) -> one block per sequence."""
    if pack.row:
        return [out[n:n + 1] for n in range(len(pack.lengths))]
    return [out[pack.cu[n]:pack.cu[n + 1]] for n in range(len(pack.lengths))]


def query_row(pack, n) -> int:
    return pack.lengths[n] - 1 if pack.mode == "last" else 0


def margins(pack):
    return [None if s is None else s.margin for s in pack.seqs]


def assert_margins(pack):
    low = [(n, m) for n, m in enumerate(margins(pack)) if m is not None and m < MIN_MARGIN]
    assert not low, f"exact-selection margin below {MIN_MARGIN} for (sequence, margin) {low}: lengths {pack.lengths}"


def selection_want(pack):
    """Per sequence v[pi]: [S_n][D], or for the row entry the one row of its query."""
    want = []
    for n, s in enumerate(pack.seqs):
        if s is None:
            want.append(None)
            continue
        sel = torch.gather(s.v, 2, s.pi[..., None].expand(-1, -1, -1, HD))           # [1][H][S][64]
        if pack.row:
            sel = sel[:, :, query_row(pack, n):query_row(pack, n) + 1]
        want.append(_rows(sel))
    return want


def selection_failures(pack, out):
    """[(sequence, what)] of the sequences whose output is not v[pi] bit for bit."""
    bad = []
    for n, (got, want) in enumerate(zip(per_sequence(pack, out), selection_want(pack))):
        if want is None:
            continue
        got = got.double()
        if bool(torch.isnan(got).any()):
            bad.append((n, f"{int(torch.isnan(got).sum())} NaN (unwritten?) elements"))
        elif not torch.equal(got, want):
            r, c = (got != want).nonzero()[0].tolist()
            bad.append((n, f"row {r} col {c}: got {float(got[r, c])} want {float(want[r, c])}"))
    return bad


def bound_ratios(pack, out):
    """Per sequence the worst |got - want| / bound against fp64 (attn16_forward) under attn16_out_bound with c_P = 1 (tiled: P
    rounded to the type) or 0 (row entry: P kept in fp32); inf for a non-finite element."""
    ratios = []
    for n, (got, s) in enumerate(zip(per_sequence(pack, out), pack.seqs)):
        if s is None:
            ratios.append(None)
            continue
        want, _, p, eps = attn16_forward(s)
        bound = attn16_out_bound(s, want, p, eps, 0.0 if pack.row else 1.0)
        g = got.double().reshape(1, -1, pack.H, HD).permute(0, 2, 1, 3)
        ratios.append(float(((g - want).abs() / bound).max()) if bool(torch.isfinite(g).all()) else float("inf"))
    return ratios


def emulate_sequence(pack, n, foreign=None):
    """The kernels' documented roundings in fp64 for sequence n: scores and softmax exact, P = exp(s - max) rounded to the type
    for P V in the tiled kernels (fp32 in the row kernel), the row sum from the unrounded P, the output rounded to the type.
    `foreign` = (k [H][64], v [H][64]): one key of ANOTHER sequence made visible to every query — what a wrong seam would do."""
    s = pack.seqs[n]
    S = pack.lengths[n]
    q, k, v = s.q, s.k, s.v
    if pack.row:
        q = q[:, :, query_row(pack, n):query_row(pack, n) + 1]
    mask = torch.zeros(q.shape[2], S, dtype=torch.float64)
    if pack.mode == "causal":
        mask = torch.full((S, S), float("-inf"), dtype=torch.float64).triu(1)
    if foreign is not None:
        k = torch.cat([k, foreign[0][None, :, None, :].double()], 2)
        v = torch.cat([v, foreign[1][None, :, None, :].double()], 2)
        mask = torch.cat([mask, torch.zeros(mask.shape[0], 1, dtype=torch.float64)], 1)
    sc = q @ k.transpose(-1, -2) * 0.125 + mask
    p = torch.exp(sc - sc.max(-1, keepdim=True).values)
    l = p.sum(-1, keepdim=True)
    pr = p if pack.row else round16(p, pack.ty).double()
    return _rows(round16((pr @ v) / l, pack.ty).double())


def emulate_pack(pack, leak=None):
    """Every sequence's emulated output, laid out as the entry writes it (an empty sequence's row: NaN).  leak = (n, k, v):
    sequence n also sees the foreign key (k, v)."""
    D = pack.H * HD
    blocks = []
    for n, s in enumerate(pack.seqs):
        if s is None:
            blocks.append(torch.full((1 if pack.row else 0, D), float("nan"), dtype=torch.float64))
        else:
            blocks.append(emulate_sequence(pack, n, leak[1:] if leak is not None and leak[0] == n else None))
    return torch.cat(blocks)


# ------------------------------------------------------------------------------------------------ the C ABI call

def entry(lib, pack):
    return getattr(lib, "dclip_" + SITES[pack.mode] % pack.tyname)


def run_pack(lib, dev, stream, pack, qkv=None, max_S=None):
    """One call of the pack's entry: qkv in the type with NaN rows behind it, the output in a guarded buffer filled with NaN.
    Returns the output [T or N][D] on the host in the type."""
    D = pack.H * HD
    src = poisoned(pack.qkv if qkv is None else qkv, 3 * D, dev, dtype=pack.ty.dtype)
    out = Guarded(out_rows(pack), D, device=dev, dtype=pack.ty.dtype)
    cu = torch.tensor(pack.cu, dtype=torch.int32, device=dev)
    site = SITES[pack.mode] % pack.tyname
    flag = int(pack.mode in ("causal", "last"))
    rc = entry(lib, pack)(src.data_ptr(), cu.data_ptr(), out.ptr, len(pack.lengths), max_S or max(pack.lengths), pack.H, flag,
                          stream)
    assert rc == 0, f"{site}: rc={rc}: {lib.dclip_last_error().decode(errors='replace')}"
    assert lib.dclip_last_launch() == site.encode(), lib.dclip_last_launch()
    torch.cuda.synchronize()
    out.assert_guards(f"{site} {pack.lengths} H={pack.H}")
    return out.get()


def bits(t):
    return t.contiguous().view(torch.int16)


def is_poison(t) -> bool:
    """Every element still holds the quiet NaN a guarded buffer's payload is filled with."""
    return bool((bits(t) == NAN16[t.dtype]).all())
