"""TEST-ONLY checkers and case lists for the fused split-fp16 GEMM entries (dclip_gemm_f16x3_*) through the C ABI
(tests/test_f16x3_paths_gpu.py, self-tested without a GPU by tests/test_kernel_checks_f16x3_cpu.py).

Built on tests/kernel_checks_split16.py: the K-major twins reuse its scaled-GEMM forms, restatement and verification — here the
contraction is the three products A_hi W_hi + A_lo W_hi + A_hi W_lo of FOUR independent integer matrices in [-2, 2], so that a
swapped, dropped or doubled product, or a computed lo.lo, changes the expected value, which stays exact in fp32 in any order.
The device operands hold NaN in every column the contract says is not read: the duplicate third of each operand and the padding
of lda / ldw.  The statistics twin is restated in the kernel's own summation order from the C it stored; the token-major twin
follows the segmented weight gradient's checker: exact C, every word of the documented slabs written, nothing behind them."""
from __future__ import annotations

from collections import namedtuple
from types import SimpleNamespace

import torch

from tests.kernel_checks import NAN, Guarded, poisoned, roundup
from tests import kernel_checks_rest as kr
from tests import kernel_checks_split16 as ks
from tests.kernel_checks_rest import Report, gen, vec

HALF = torch.float16
X3_SHAPES = [(257, 260), (300, 264), (511, 520)]       # the ping-pong shapes of the scaled entries: 4, 4 and 6 tiles of 256 x 256
X3_K = [32, 64, 96, 160]                               # 1 K-tile (prologue only), both buffers, an odd count, the last-tile waits
X3_FORMS = dict(ks.GEMM_FORMS)
X3_FORMS["rows_stats"] = dict(fn="rows_stats", epi=0)
X3_FORMS["rows_stats_dgelu"] = dict(fn="rows_stats", epi=ks.EPI_DGELU)
X3_ENTRIES = tuple(X3_FORMS)
X3_NAMES = {"scaled": "gemm_f16x3_scaled", "scaled_dev": "gemm_f16x3_scaled_dev", "rows_dev": "gemm_f16x3_scaled_rows_dev",
            "split": "gemm_f16x3_scaled_split", "split_dev": "gemm_f16x3_scaled_split_dev",
            "rows_stats": "gemm_f16x3_scaled_rows_dev.stats"}
X3Case = namedtuple("X3Case", "entry M N K cpad perm")
PRODUCT_FAULTS = ("product_dropped", "product_doubled", "product_swapped", "lo_lo_added", "duplicate_read", "padding_read")


def x3_cases():
    """Every entry form at every K, the shape, the padding of C and the segment order rotating."""
    out = []
    for j, e in enumerate(X3_ENTRIES):
        for i, K in enumerate(X3_K):
            M, N = X3_SHAPES[(i + j) % 3]
            out.append(X3Case(e, M, N, K, 1 if X3_FORMS[e]["epi"] & ks.EPI_DGELU else (i + j) % 2, bool((i + j // 3) % 2)))
    return out


def x3_id(c) -> str:
    return f"{c.entry}-{c.M}x{c.N}x{c.K}-pad{c.cpad}-{'perm' if c.perm else 'step'}"


def x3_site(c) -> str:
    return X3_NAMES[X3_FORMS[c.entry]["fn"]] + ".pp3"


def x3_form(c):
    f = dict(split=False, g32=False, h32=False, noscale=False, big=False, negzero=False)
    f.update(X3_FORMS[c.entry])
    return SimpleNamespace(**f)


def x3_offsets(c):
    """(a_hi, a_lo, w_hi, w_lo): the step's layout — A = [hi|lo|hi], W = [hi|hi|lo] — or another one; the third K columns of each
    operand are never read."""
    K = c.K
    return (2 * K, 0, K, 0) if c.perm else (0, K, 0, 2 * K)


def _place(pieces, offs, K, rows):
    m = torch.full((rows, 3 * K), NAN)
    for p, o in zip(pieces, offs):
        m[:, o:o + K] = p
    return m


def build_x3(c: X3Case, device="cpu"):
    f = x3_form(c)
    seed = 1000 * c.M + 10 * c.N + c.K
    M, N, K = c.M, c.N, c.K
    ah, al, wh, wl = (kr.ints(sh, seed + 10 + i) for i, sh in enumerate([(M, K), (M, K), (N, K), (N, K)]))
    bias = torch.randint(-4096, 4097, (N,), generator=gen(seed + 2)).float() * 2.0 ** -12
    ra = torch.exp2((torch.arange(M) % 13 - 6).float())
    alpha = 2.0 ** ks.GEMM_ALPHA_EXP
    if f.big:                                              # sums of multiples of 2^25 below 2^25 2^24: exact
        ah, al = (torch.randint(0, 2, (M, K), generator=gen(seed + i)).float() * 8192.0 + 8192.0 for i in (10, 11))
        wh, wl = (torch.randint(0, 2, (N, K), generator=gen(seed + i)).float() * 4096.0 + 4096.0 for i in (12, 13))
        ra = torch.where(torch.arange(M) % 2 == 0, 2.0 ** 100, 2.0 ** -60).float()
        alpha = 2.0 ** ks.GEMM_BIG_ALPHA_EXP
    if f.negzero:
        alpha = -alpha
        wh[:4] = 0.0
        wl[:4] = 0.0
        bias[:4] = -0.0
    # the host form of the three products as ONE contraction, for kernel_checks_split16's restatement: [hi|lo|hi] with [hi|hi|lo]
    a, w = torch.cat([ah, al, ah], 1), torch.cat([wh, wh, wl], 1)
    lda = ldw = 3 * K + 8
    rows = f.fn in ("rows_dev", "rows_stats")
    ldc = roundup(3 * N, 8) + 8 * c.cpad if f.split else N + 4 * c.cpad
    if f.noscale:
        ldc = roundup(N, 8) + 8 * c.cpad
    res = kr.ints((M, N), seed + 3)
    lin = (ah.double() @ wh.double().t() + al.double() @ wh.double().t() + ah.double() @ wl.double().t()) * alpha
    if rows:
        lin = lin * ra.double()[:, None]
    if f.epi & ks.EPI_BIAS:
        lin = lin + bias.double()
    if f.epi & ks.EPI_RESIDUAL:
        lin = lin + res.double()
    assert torch.equal(lin.float().double(), lin)                  # every expected linear value is exactly representable in fp32
    aux = torch.randint(-8, 9, (M, N), generator=gen(seed + 4)).float() * 0.5 if f.epi & ks.EPI_DGELU else None
    offs = x3_offsets(c)
    P = -(-M // 256)
    s = SimpleNamespace(case=c, form=f, a=a, w=w, pieces=(ah, al, wh, wl), offs=offs, bias=bias, res=res, ra=ra, lin=lin, want=lin,
                        epi=f.epi, lda=lda, ldw=ldw, ldc=ldc, alpha_v=alpha, aux=aux,
                        A=poisoned(_place((ah, al), offs[:2], K, M), lda, device, dtype=HALF),
                        W=poisoned(_place((wh, wl), offs[2:], K, N), ldw, device, dtype=HALF),
                        bias_d=torch.cat([bias, torch.full((8,), NAN)]).to(device),
                        res_d=poisoned(res, ldc, device) if f.epi & ks.EPI_RESIDUAL else None,
                        aux_d=poisoned(aux, ldc, device) if aux is not None else None,
                        ra_d=vec(M, device, fill=ra[None]), alpha=vec(1, device, fill=alpha),
                        out_scale=vec(1, device, fill=2.0 ** ks.GEMM_OUT_EXP),
                        C=Guarded(M, 3 * N if f.split else N, ldc, device=device, dtype=HALF if f.split else torch.float32),
                        g32=Guarded(M, N, device=device) if f.g32 else None,
                        h32=Guarded(M, N, device=device) if f.h32 else None,
                        pmax=Guarded(P, N, device=device, dtype=torch.float32) if f.fn == "rows_stats" else None,
                        psum=Guarded(P, N, device=device) if f.fn == "rows_stats" else None)
    return s


def launch_x3(lib, s, stream, K=None, offs=None, lda=None, ldw=None) -> int:
    """The fused entry of the case; the keyword arguments override one argument each (the refusals)."""
    c, f = s.case, s.form
    A, W, C, b = s.A.data_ptr(), s.W.data_ptr(), s.C.ptr, s.bias_d.data_ptr()
    r = None if s.res_d is None else s.res_d.data_ptr()
    dims = (c.M, c.N, c.K if K is None else K, s.lda if lda is None else lda, s.ldw if ldw is None else ldw, s.ldc,
            *(s.offs if offs is None else offs))
    aux = None if s.aux_d is None else s.aux_d.data_ptr()
    if f.fn == "scaled":
        return lib.dclip_gemm_f16x3_scaled(A, W, C, b, r, *dims, f.epi, 0, s.alpha_v, stream)
    if f.fn == "scaled_dev":
        return lib.dclip_gemm_f16x3_scaled_dev(A, W, C, b, r, *dims, f.epi, 0, s.alpha.ptr, stream)
    if f.fn == "rows_dev":
        return lib.dclip_gemm_f16x3_scaled_rows_dev(A, W, C, aux, *dims, f.epi, s.alpha.ptr, s.ra_d.ptr, stream)
    if f.fn == "rows_stats":
        return lib.dclip_gemm_f16x3_scaled_rows_stats_dev(A, W, C, aux, *dims, f.epi, s.alpha.ptr, s.ra_d.ptr, s.pmax.ptr, s.psum.ptr,
                                                          stream)
    if f.fn == "split":
        return lib.dclip_gemm_f16x3_scaled_split(A, W, C, b, *dims, f.epi, s.alpha_v, 2.0 ** ks.GEMM_OUT_EXP, stream)
    hp = s.h32.ptr if s.h32 is not None else None
    gp = s.g32.ptr if s.g32 is not None else None
    op = None if f.noscale else s.out_scale.ptr
    return lib.dclip_gemm_f16x3_scaled_split_dev(A, W, C, b, hp, gp, *dims, f.epi, s.alpha.ptr, op, stream)


def tile_stats(C: torch.Tensor):
    """(pmax, psum) [ceil(M / 256)][N] of a stored fp32 C [M][N] as the ping-pong epilogue forms them: the maximum of the bit
    patterns of |v|; the fp32 sum in the kernel's order — thread row w = 0..7 of a tile adds its rows 128 hm + w + 8 q (hm = 0, 1;
    q = 0..15) in turn, then the eight partial sums are folded in order."""
    C = C.detach().cpu().float()
    M, N = C.shape
    P = -(-M // 256)
    pmax = torch.zeros((P, N), dtype=torch.int32)
    psum = torch.zeros((P, N))
    for t in range(P):
        blk = C[256 * t:256 * (t + 1)]
        pmax[t] = (blk.view(torch.int32) & 0x7FFFFFFF).amax(dim=0)
        parts = []
        for w in range(8):
            acc = torch.zeros(N)
            for hm in range(2):
                for q in range(16):
                    r = 128 * hm + w + 8 * q
                    if r < blk.shape[0]:
                        acc = acc + blk[r]
            parts.append(acc)
        sm = parts[0]
        for w in range(1, 8):
            sm = sm + parts[w]
        psum[t] = sm
    return pmax, psum


def emulate_x3(s, fault=None):
    """kernel_checks_split16's restatement of the entry on the three products; `fault` plants one defect in the contraction (the
    epilogue faults are that module's own)."""
    ah, al, wh, wl = s.pieces
    keep = s.a, s.w
    if fault == "product_dropped":
        s.a, s.w = torch.cat([ah, al], 1), torch.cat([wh, wh], 1)
    elif fault == "product_doubled":
        s.a, s.w = torch.cat([ah, al, ah, ah], 1), torch.cat([wh, wh, wl, wh], 1)
    elif fault == "product_swapped":                       # lo.lo in the place of hi.lo
        s.a, s.w = torch.cat([ah, al, al], 1), torch.cat([wh, wh, wl], 1)
    elif fault == "lo_lo_added":
        s.a, s.w = torch.cat([ah, al, ah, al], 1), torch.cat([wh, wh, wl, wl], 1)
    elif fault == "duplicate_read":                        # the third K columns of A as the device holds them
        dup = s.A[:s.case.M, :3 * s.case.K].float().cpu()
        third = [o for o in (0, s.case.K, 2 * s.case.K) if o not in s.offs[:2]][0]
        s.a, s.w = torch.cat([ah, al, dup[:, third:third + s.case.K]], 1), torch.cat([wh, wh, wl], 1)
    elif fault == "padding_read":
        s.a, s.w = torch.cat([ah, al, ah], 1), torch.cat([wh, wh, wl], 1)
        s.a[:, -1] = s.A[:s.case.M, 3 * s.case.K].float().cpu()
    form = s.form
    if form.fn == "rows_stats":                            # the row-scaled entry's arithmetic
        s.form = SimpleNamespace(**{**vars(form), "fn": "rows_dev"})
    ks.emulate_scaled(s, fault if fault not in PRODUCT_FAULTS else None)
    s.form = form
    s.a, s.w = keep
    if s.pmax is not None:
        pm, ps = tile_stats(s.C.get())
        if fault == "stats_all_rows":                      # the maxima taken over the tile's 256 rows, those behind M included
            pm[-1] = torch.maximum(pm[-1], torch.full_like(pm[-1], 0x7FC00000))
        if fault == "stats_sum_order":
            ps = torch.stack([s.C.get()[256 * t:256 * (t + 1)].flip(0).double().sum(0) * (1 + 2.0 ** -20) for t in range(ps.shape[0])]).float()
        s.pmax.payload.copy_(pm.view(torch.float32))
        s.psum.payload.copy_(ps)


def verify_x3(s, what=None):
    fig = ks.verify_scaled(s, what or x3_id(s.case))
    if s.pmax is not None:
        rep = Report((what or x3_id(s.case)) + " statistics")
        rep.guards(pmax=s.pmax, psum=s.psum)
        pm, ps = tile_stats(s.C.get())
        if not torch.equal(kr.ibits(s.pmax.get()), pm):
            rep.fail("pmax: not the maxima of the bit patterns of |C| over each tile's rows")
        if s.epi & ks.EPI_DGELU:
            # the compiler may contract the DGELU product into the sum (an fma on the unrounded product), so the sums are those of
            # the stored values only up to rounding: 256 additions and one product rounding per term, (256 + 1) 2^-24 sum |v|
            C = s.C.get().double()
            blocks = [C[256 * t:256 * (t + 1)] for t in range(ps.shape[0])]
            rep.bound("psum", s.psum.get(), torch.stack([b.sum(0) for b in blocks]),
                      257 * 2.0 ** -24 * torch.stack([b.abs().sum(0) for b in blocks]) + 2.0 ** -126)
        else:
            rep.bits("psum", s.psum.get(), ps)
        fig.update(rep.done())
    return fig


# ==================================================================================================== the token-major twin

TOK_SIZES, TOK_TOKENS, TOK_SPLITS = list(ks.SEG_SIZES), [64, 128, 192, 1088], [1, 2, 3]
TOK_SITE = "gemm_f16x3_wgrad_tokmajor.pp3_tok.splitk_reduce"
TokCase = namedtuple("TokCase", "M N tokens splits perm")


def tok_cases():
    """Every (tokens, splits) pair on three of the nine (M, N), rotating, with both sets of segments."""
    out = []
    sizes = [(m, n) for m in TOK_SIZES for n in TOK_SIZES]
    for i, tokens in enumerate(TOK_TOKENS):
        for k, splits in enumerate(TOK_SPLITS):
            for j in range(3):
                M, N = sizes[(3 * k + j + 3 * i) % 9]
                out.append(TokCase(M, N, tokens, splits, bool((i + k + j) % 2)))
    return out


def tok_id(c) -> str:
    return f"{c.M}x{c.N}-tok{c.tokens}-s{c.splits}-{'perm' if c.perm else 'step'}"


def tok_offsets(c):
    """(dy_hi, dy_lo, x_hi, x_lo): the step's — dY = [hi|lo], X = [hi|lo|hi] — or another set; X's remaining third is never read."""
    return (c.M, 0, 2 * c.N, 0) if c.perm else (0, c.M, 0, c.N)


def build_tok(c: TokCase, device="cpu"):
    seed = 1000 * c.M + 10 * c.N + c.tokens + c.splits
    lddy, ldx = 2 * c.M + 8, 3 * c.N + 16
    dyh, dyl, xh, xl = (kr.ints(sh, seed + i) for i, sh in enumerate([(c.tokens, c.M)] * 2 + [(c.tokens, c.N)] * 2))
    offs = tok_offsets(c)
    dy = torch.full((c.tokens, 2 * c.M), NAN)
    x = torch.full((c.tokens, 3 * c.N), NAN)
    dy[:, offs[0]:offs[0] + c.M], dy[:, offs[1]:offs[1] + c.M] = dyh, dyl
    x[:, offs[2]:offs[2] + c.N], x[:, offs[3]:offs[3] + c.N] = xh, xl
    ca = torch.exp2(((torch.arange(c.M) * 7) % 41 - 20).float())
    _, s_eff = ks.seg_s_eff(c.tokens, c.splits)
    floats = s_eff * c.M * c.N
    return SimpleNamespace(case=c, pieces=(dyh, dyl, xh, xl), offs=offs, ca=ca, s_eff=s_eff, lddy=lddy, ldx=ldx,
                           dyd=poisoned(dy, lddy, device, dtype=HALF), xd=poisoned(x, ldx, device, dtype=HALF),
                           cad=vec(c.M, device, fill=ca[None]), act=vec(1, device, fill=2.0 ** ks.SEG_ACT_EXP),
                           C=Guarded(c.M, c.N, c.N + 4, device=device), ws=vec(floats + kr.WS_TAIL, device), ws_bytes=4 * floats)


def launch_tok(lib, s, stream, ws_bytes=None) -> int:
    c = s.case
    return lib.dclip_gemm_f16x3_wgrad_tokmajor(s.dyd.data_ptr(), s.xd.data_ptr(), s.C.ptr, c.M, c.N, c.tokens, s.lddy, s.ldx, s.C.ld,
                                               *s.offs, s.cad.ptr, s.act.ptr, c.splits, s.ws.ptr,
                                               s.ws_bytes if ws_bytes is None else ws_bytes, stream)


def emulate_tok(s, fault=None):
    """s_eff fp32 slabs, one per token range, each the three products of its tokens; then their sum in order, divided by the
    activation scale, times col_alpha."""
    c = s.case
    dyh, dyl, xh, xl = s.pieces
    kps, s_eff = ks.seg_s_eff(c.tokens, c.splits)
    slabs = s.ws.payload[0, :s_eff * c.M * c.N].view(s_eff, c.M, c.N)
    for k in range(s_eff):
        r = slice(k * kps, (k + 1) * kps)
        v = dyh[r].t() @ xh[r] + dyl[r].t() @ xh[r]
        if fault != "product_dropped":
            v = v + (dyl if fault == "product_swapped" else dyh)[r].t() @ xl[r]
        if fault == "lo_lo_added":
            v = v + dyl[r].t() @ xl[r]
        if fault == "tokens_shifted" and k == s_eff - 1:   # the lo pieces of the NEXT 32 tokens
            sh = torch.cat([xl[r][32:], xl[r][:32]])
            v = dyh[r].t() @ xh[r] + dyl[r].t() @ xh[r] + dyh[r].t() @ sh
        slabs[k] = v
    acc = torch.zeros((c.M, c.N))
    for k in range(s_eff - (1 if fault == "slab_left_out" else 0)):
        acc = acc + slabs[k]
    s.C.payload.copy_((acc * 2.0 ** -ks.SEG_ACT_EXP) * s.ca[:, None])
    if fault == "slab_unwritten":
        slabs[s_eff - 1, c.M - 1, c.N - 1] = NAN
    if fault == "ws_behind":
        s.ws.payload[0, s_eff * c.M * c.N] = 0.0
    if fault == "c_pad":
        s.C.mat[0, c.N] = 0.0


def verify_tok(s, what=None):
    c = s.case
    rep = Report(what or f"f16x3_wgrad_tokmajor {tok_id(c)}")
    rep.guards(C=s.C, workspace=s.ws, col_alpha=s.cad, act_scale=s.act)
    dyh, dyl, xh, xl = (t.double() for t in s.pieces)
    acc = dyh.t() @ xh + dyl.t() @ xh + dyh.t() @ xl
    want = acc * 2.0 ** -ks.SEG_ACT_EXP * s.ca.double()[:, None]
    assert torch.equal(want.float().double(), want)                # every expected value is exactly representable in fp32
    rep.exact("C", s.C.get(), want)
    ws = s.ws.get()[0]
    used = s.s_eff * c.M * c.N
    if bool(torch.isnan(ws[:used]).any()):
        rep.fail(f"workspace: {int(torch.isnan(ws[:used]).sum())} words of the {s.s_eff} slabs were never written")
    if not bool(torch.isnan(ws[used:]).all()):
        rep.fail(f"workspace: wrote behind its documented size ({int((~torch.isnan(ws[used:])).sum())} of {kr.WS_TAIL} floats)")
    return rep.done()


# ==================================================================================================== real split data

def split_bound(ah, al, wh, wl, K: int):
    """The any-order bound of 3 K exact products accumulated in fp32: 3 K 2^-23 (|A_hi||W_hi| + |A_lo||W_hi| + |A_hi||W_lo|), and
    the fp64 value of the three products; operands [M][K] and [N][K]."""
    ah, al, wh, wl = (t.double() for t in (ah, al, wh, wl))
    want = ah @ wh.t() + al @ wh.t() + ah @ wl.t()
    mag = ah.abs() @ wh.abs().t() + al.abs() @ wh.abs().t() + ah.abs() @ wl.abs().t()
    return want, 3 * K * 2.0 ** -23 * mag
