"""Kernel parity on the long-row routes (>= 2^18 rows) against fp64.

At the row counts of the headline step's 256^2 and 128^2 stages (524288 and 2097152 rows at
B = 32) the launchers switch plans on plain row-count tests that no small shape can reach
(the production library folds every development slot to 0).  Each case below sits at the
smallest shape that takes its route, or just past it with a row count that is no multiple of
the chunk or tile, so that the persistent loops' last trip is partly out of range.

Route inventory (entry point | shape, bf16 unless noted | route it must take | source).
"family" routes are asserted through L.launched_kernels(); the noted names carry no template
values, so routes that differ only by instantiation or block cap are pinned by the shape alone.

 W1 edet_conv1x1_wgrad   | 262144 x 16 -> 96, x 32 -> 16, plain A | k_wgs + k_sum_partials (family)          | gemm.hip:2578
 W2 edet_conv1x1_wgrad   | 263500 x 24 -> 40 (ragged), plain A    | k_wgs, last row group partly out of range | gemm.hip:2578
 W3 edet_conv1x1_wgrad   | 524288 x 24 -> 144, plain A            | k_wgrad_tr, min_stages 16, partials (3 tiles, split 512; family) | gemm.hip:2617-2629
 W4 edet_conv1x1_wgrad   | 524288 x 144 -> 24, gated swish(bn) A  | k_wgrad_tr lazy, partials (family)        | gemm.hip:2617-2629
 W5 edet_conv1x1_wgrad   | 524288 x 96 -> 144, plain A            | k_wgrad_tr, min_stages 16, atomics (6 tiles; family) | gemm.hip:2617, 2628
 W6 edet_conv1x1_wgrad   | 528066 x 24 -> 144 (ragged), plain A   | k_wgrad_tr, partials, ragged last stage   | gemm.hip:2617-2629
 G1 edet_conv1x1_fwd     | 2097152 x 32 -> 16, gated swish(bn) A  | k_gemm_s (family), 1024-block cap (shape) | gemm.hip:2067
 G2 edet_conv1x1_fwd     | 2097152 x 16 -> 96, plain A            | k_gemm_s (family), 1024-block cap (shape) | gemm.hip:2067
 G3 edet_conv1x1_fwd     | 2103750 x 32 -> 16 (ragged), plain A   | k_gemm_s, last 16-row group partly out    | gemm.hip:2067
 G4 edet_conv1x1_dgrad, edet_conv1x1_dgrad_fold | 2097152 x 96 -> 16 | k_gemm_s (family), 1024-block cap (shape) | gemm.hip:2067, 2316
 G5 edet_conv1x1_fwd     | 524288 x 144 -> 24, plain A, statistics | k_gemm_s (family), 512 blocks past the 256-block cap's 262144 rows (shape) | gemm.hip:2066
 A1 edet_lazy_bwd_apply  | 524288 x 24, x 144; 528066 x 24        | nontemporal instantiation (shape; bf16, accumulate 0) | bn.hip:955
 A2 edet_lazy_bwd_apply  | 524288 x 144, no gate                  | 512-block persistent grid (shape)         | bn.hip:947
 A3 edet_lazy_bwd_apply  | 524288 x 96, SE gate                   | nontemporal, 8 passes, 2048-block grid (shape) | bn.hip:923, 947, 955
 R1 edet_lazy_bwd_reduce | 524288 x 24                            | 1024-block cap (shape)                    | bn.hip:892
 R2 edet_lazy_bwd_reduce | 528066 x 24 (ragged, M > 524288)       | 256-block cap (shape)                     | bn.hip:892
 R3 edet_lazy_bwd_reduce | 524288 x 144, one segment              | 32-pass plan (shape)                      | bn.hip:884
 M1 edet_lazy_materialize| 524288 x 144; 528066 x 144             | 8-pass plan (shape)                       | bn.hip:1125
 D1 edet_dwconv_fwd      | k3 s1, 524288 x 24; 528066 x 24        | k_dws (family), 2x block target (shape)   | dwconv.hip:1498
 D2 edet_dwconv_fwd      | k3 s2, 2097152 x 96                    | k_dws (family), 4x block target (shape)   | dwconv.hip:1501
 D3 edet_dwconv_bwd      | k3 s1, 524288 x 24; 528066 x 24        | k_dwb (family: C % 16 != 0 keeps bf16 off the tiled k_dwt), 2x target (shape) | dwconv.hip:2440
 D4 edet_dwconv_dgrad_fold | k3 s2, 1048576 x 32; 1083750 x 32; pyramid | k_dw4_dgrad alone, no reduce pass (family) | dwconv.hip:2695
 D5 edet_dwconv_dgrad    | k3 s2, 1048576 x 32 (> 131072 rows)    | k_dw4_dgrad (family), 4096-block cap (shape) | dwconv.hip:1077
 S1 edet_se_squeeze, edet_gate_grad | B x H*W x C = 32 x 16384 x 144 | 16 passes kept (B * chunks >= 512; shape) | bn.hip:980
 S2 edet_se_squeeze, edet_gate_grad | 8 x 65536 x 16, 3 x 65536 x 32, 5 x 16383 x 96 | halving ends at 8 / at the floor 4 (shape) | bn.hip:980
 S3 edet_gate_bn_reduce  | the four shapes of S1 / S2             | 32 passes kept / halved to 8 / to 4 (shape) | bn.hip:1026

Checks.  Element-wise outputs: the destination is prefilled with NaN, the kernel runs twice
and (no atomics) must give identical bits, and the result is compared with fp64 at gpu_util.TOL
with the scales of test_kernels_large_gpu.py.  Sums of the bf16-only routes (k_wgs, k_wgrad_tr,
k_gemm_s) also have an exact case: every operand is a small integer, so every product and
partial sum is an integer; with rows * max|term| < 2^24 fp32 addition is exact in any order (the
fp64 destinations too) and the result must equal the fp64 reference bit for bit -- a dropped
or doubled row group cannot hide inside a sqrt(n) bar.  Outputs that stay on tolerance there:
the sum of y^2 of the forward statistics (rows * max y^2 passes 2^24) and dgamma of the BN
backward (xhat is no integer; the fp32 instantiation of the same template guards it).

fp64 references are built in row blocks (gpu_util.row_blocks) or per image.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from tf2mv_amd import _lib as L
from tf2mv_amd.runtime import Pyr, ensure_workspace, stream, vp
from gpu_util import (DEV, DT, TDT, BnBwdClosedForm, LazyDesc, bngrad64, close, dswish, g, ints, make_bn, ref_threads,
                      routed, row_blocks, stat_out, stats_out, zeros, zeros64)

DTS = ["f32", "bf16"]
EXACT = 1 << 24  # integers below this add exactly in fp32, in any order


@pytest.fixture(autouse=True)
def _setup(request):
    if "gpu" in request.keywords:
        ensure_workspace(DEV)  # the split-reduction workspace the model registers (partials routes)
    ref_threads()


def rnd(rng, *shape, scale=1.0):
    return torch.tensor(rng.standard_normal(shape, dtype=np.float32) * scale)


def nan_like(rows, C, dt):
    return torch.full((rows, C), float("nan"), dtype=TDT[dt], device=DEV)


def bn_tables(bn):
    return tuple(t.double().cpu() for t in bn[0])


# ----------------------------------------------------------------- the closed form itself (CPU)
def test_bn_bwd_closed_form_equals_autograd():
    """The blocked closed-form BN backward the long-row references use, against fp64 autograd
    through batch statistics recomputed from x, to 1e-10 relative."""
    rng = np.random.default_rng(11)
    n, C = 777, 24
    for act in (0, 1):
        x = torch.tensor(rng.standard_normal((n, C)) * 2 + 0.3, dtype=torch.float64)
        dv = torch.tensor(rng.standard_normal((n, C)), dtype=torch.float64)
        ga = torch.tensor(rng.uniform(0.5, 1.5, C)).requires_grad_(True)
        be = torch.tensor(rng.uniform(-0.5, 0.5, C)).requires_grad_(True)
        xr = x.clone().requires_grad_(True)
        mean = xr.mean(0)
        var = ((xr - mean) ** 2).mean(0)
        u = (xr - mean) / torch.sqrt(var + 1e-3) * ga + be
        ((u * torch.sigmoid(u) if act else u) * dv).sum().backward()
        cf = BnBwdClosedForm(x.sum(0), (x * x).sum(0), ga.detach(), be.detach(), n, act=act)
        blocks = row_blocks(0, n, 200)
        for b in blocks:
            cf.add(x[b], dv[b])
        dx = torch.cat([cf.dx(x[b], dv[b]) for b in blocks])
        for got, ref in ((dx, xr.grad), (cf.dbeta, be.grad), (cf.dgamma, ga.grad)):
            assert float((got - ref).abs().max()) <= 1e-10 * float(ref.abs().max())


# ----------------------------------------------------------------- conv1x1 weight gradient
WGRAD = [  # row, B, H, W, K, N, lazy, family, sum pass
    ("W1", 16, 128, 128, 16, 96, 0, "k_wgs", True), ("W1", 16, 128, 128, 32, 16, 0, "k_wgs", True),
    ("W2", 17, 125, 124, 24, 40, 0, "k_wgs", True),
    ("W3", 32, 128, 128, 24, 144, 0, "k_wgrad_tr", True), ("W4", 32, 128, 128, 144, 24, 1, "k_wgrad_tr", True),
    ("W5", 32, 128, 128, 96, 144, 0, "k_wgrad_tr", False), ("W6", 33, 127, 126, 24, 144, 0, "k_wgrad_tr", True)]


@pytest.mark.gpu
@pytest.mark.parametrize("row,B,H,W,K,N,lazy,family,sum_pass", WGRAD)
def test_conv1x1_wgrad_long(row, B, H, W, K, N, lazy, family, sum_pass):
    """bf16 dW / db of the wave-streaming form and of the transposing tiles over M >= 524288.
    Plain operands are integers of [-2, 2]: dW and db must equal fp64 exactly.  The lazy A
    (W4) is compared at the bar of test_conv1x1_wgrad_large."""
    rng = np.random.default_rng(K * 7 + N + B)
    pyr = Pyr(B, [(H, W)])
    M = pyr.rows
    if lazy:
        x = g(rnd(rng, M, K), "bf16")
        lz = LazyDesc(x, pyr, K, bn=make_bn(x, pyr, K, rng), act=1, gate=g(torch.rand(B, K), "f32"))
        dy = g(rnd(rng, M, N), "bf16")
    else:
        x, dy = ints(rng, (M, K), -2, 2, "bf16"), ints(rng, (M, N), -2, 2, "bf16")
        lz = LazyDesc(x, pyr, K)
        assert M * 2 * 2 < EXACT
    dw, db = zeros(N, K), zeros(N)
    names = routed("edet_conv1x1_wgrad", L.BF16, lz.c, pyr.c, K, vp(dy), N, N, vp(dw), vp(db), stream())
    assert family in names and not ({"k_wgs", "k_wgrad_tr", "k_wgrad"} - {family}) & set(names), (row, names)
    assert ("k_sum_partials" in names) == sum_pass, (row, names)
    refw = torch.zeros(N, K, dtype=torch.float64)
    refb = torch.zeros(N, dtype=torch.float64)
    for b in row_blocks(0, M):
        d = dy[b].double().cpu()
        refw += d.t() @ lz.cpu_rows(b)
        refb += d.sum(0)
    if lazy:
        close(dw, refw, "bf16", scale=M ** 0.5 * 2)
        close(db, refb, "bf16", scale=M ** 0.5 * 2)
    else:
        assert torch.equal(dw.double().cpu(), refw), f"{row}: dW max diff {float((dw.double().cpu() - refw).abs().max())}"
        assert torch.equal(db.double().cpu(), refb), f"{row}: db max diff {float((db.double().cpu() - refb).abs().max())}"


# ----------------------------------------------------------------- conv1x1 forward / dgrad over 2M rows
def sparse_weight(rng, N, K, nz=3):
    """[N, K] of 0 / +-1 with nz nonzeros per output row: |x . w| <= nz for x of {-1, 0, 1}."""
    w = torch.zeros(N, K)
    for n in range(N):
        w[n, rng.choice(K, size=nz, replace=False)] = torch.tensor(rng.choice([-1.0, 1.0], size=nz), dtype=torch.float32)
    return w


@pytest.mark.gpu
@pytest.mark.parametrize("row,B,H,W,K,N,lazy", [("G1", 32, 256, 256, 32, 16, 1), ("G2", 32, 256, 256, 16, 96, 0),
                                                ("G3", 33, 255, 250, 32, 16, 0), ("G5", 32, 128, 128, 144, 24, 0)])
def test_conv1x1_fwd_long(row, B, H, W, K, N, lazy):
    """bf16 forward with BN statistics over >= 2^21 rows (k_gemm_s under its 1024-block cap; G5:
    524288 rows of the deeper plain A, past the 256-block cap of the short tensors).
    Plain cases: x of {-1, 0, 1}, three +-1 weights per output, bias of {-1, 0, 1}, so |y| <= 4
    and sum y is exact; sum y^2 stays on the bar of test_conv1x1_fwd_large."""
    rng = np.random.default_rng(K * 31 + N + B)
    pyr = Pyr(B, [(H, W)])
    M = pyr.rows
    if lazy:
        x = g(rnd(rng, M, K), "bf16")
        lz = LazyDesc(x, pyr, K, bn=make_bn(x, pyr, K, rng), act=1, gate=g(torch.rand(B, K), "f32"))
        w, b = g(rnd(rng, N, K, scale=1 / math.sqrt(K)), "bf16"), g(rnd(rng, N), "f32")
    else:
        x = ints(rng, (M, K), -1, 1, "bf16")
        lz = LazyDesc(x, pyr, K)
        w, b = g(sparse_weight(rng, N, K), "bf16"), ints(rng, (N,), -1, 1, "f32")
        assert M * 4 < EXACT
    ys, sts = [], []
    for _ in range(2):
        y, st = nan_like(M, N, "bf16"), stats_out(1, N)
        names = routed("edet_conv1x1_fwd", L.BF16, lz.c, pyr.c, K, vp(w), N, vp(b), vp(y), N, 0, stat_out(st), stream())
        assert names == ["k_gemm_s"], (row, names)
        ys.append(y)
        sts.append(st)
    torch.cuda.synchronize()
    assert torch.equal(ys[0].view(torch.int16), ys[1].view(torch.int16)), f"{row}: output differs between runs"
    wc, bc = w.double().cpu().t(), b.double().cpu()
    rs, rq = torch.zeros(N, dtype=torch.float64), torch.zeros(N, dtype=torch.float64)
    for blk in row_blocks(0, M):
        ref = lz.cpu_rows(blk) @ wc + bc
        close(ys[0][blk], ref, "bf16")
        rs += ref.sum(0)
        rq += (ref * ref).sum(0)
    if lazy:
        close(sts[0][0][0], rs, "bf16", scale=M ** 0.5 * 4)
    else:
        assert torch.equal(sts[0][0][0].v.cpu(), rs), f"{row}: sum y max diff {float((sts[0][0][0].v.cpu() - rs).abs().max())}"
    close(sts[0][0][1], rq, "bf16", scale=M ** 0.5 * 8, rtol=5e-2)


@pytest.mark.gpu
def test_conv1x1_dgrad_long():
    """G4: the 2M x 96 -> 16 dgrad, plain and with the BN-backward fold of the value dx is the
    gradient of (bn only, so du = dx).  dy of {-1, 0, 1} and three +-1 weights per dx column:
    |dx| <= 3, the fold's dbeta = sum dx is exact; dgamma at the bar of test_conv1x1_dgrad_fold."""
    rng = np.random.default_rng(96)
    B, H, W, N, K = 32, 256, 256, 96, 16
    pyr = Pyr(B, [(H, W)])
    M = pyr.rows
    dy = ints(rng, (M, N), -1, 1, "bf16")
    w = sparse_weight(rng, K, N).t().contiguous()  # [N, K]
    wkn = g(w.t().contiguous(), "bf16")  # the transposed compute copy the dgrad GEMM consumes
    x = g(rnd(rng, M, K, scale=2.0), "bf16")
    bn = make_bn(x, pyr, K, rng)
    lz = LazyDesc(x, pyr, K, bn=bn, act=0)
    assert M * 3 < EXACT
    dxs = []
    for fold in (False, True, True):
        dx = nan_like(M, K, "bf16")
        if fold:
            acc_t, acc = bngrad64(1, K)
            names = routed("edet_conv1x1_dgrad_fold", L.BF16, vp(dy), N, pyr.c, N, vp(wkn), K, vp(dx), K, lz.c, acc, stream())
        else:
            names = routed("edet_conv1x1_dgrad", L.BF16, vp(dy), N, pyr.c, N, vp(wkn), K, vp(dx), K, 0, stream())
        assert names == ["k_gemm_s"], names
        dxs.append(dx)
    torch.cuda.synchronize()
    assert torch.equal(dxs[0].view(torch.int16), dxs[1].view(torch.int16))
    assert torch.equal(dxs[1].view(torch.int16), dxs[2].view(torch.int16)), "output differs between runs"
    su, sq, ga, be = bn_tables(bn)
    cf = BnBwdClosedForm(su, sq, ga, be, M)
    wc = w.double()
    for blk in row_blocks(0, M):
        ref = dy[blk].double().cpu() @ wc
        close(dxs[0][blk], ref, "bf16")
        cf.add(x[blk].double().cpu(), ref)
    assert torch.equal(acc_t[1, 0].cpu(), cf.dbeta), f"dbeta max diff {float((acc_t[1, 0].cpu() - cf.dbeta).abs().max())}"
    close(acc_t[0, 0], cf.dgamma, "bf16", scale=M ** 0.5)


# ----------------------------------------------------------------- BN backward (reduce + apply), materialize
@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("rows,B,H,W,C,act,gate", [("A1 R1", 32, 128, 128, 24, 0, 0), ("A1 R2", 33, 127, 126, 24, 0, 0),
                                                   ("A3", 32, 128, 128, 96, 1, 1), ("A1 A2 R3", 32, 128, 128, 144, 0, 0)])
def test_lazy_bwd_long(dt, rows, B, H, W, C, act, gate):
    """edet_lazy_bwd_reduce + edet_lazy_bwd_apply over >= 524288 rows against the closed-form
    fp64 BN backward.  Where the value has no activation and no gate, dv is integers of [-2, 2]
    and dbeta = sum dv must be exact (both dtypes); dgamma at the bar of test_lazy_bwd_large."""
    rng = np.random.default_rng(C + 5 + B)
    pyr = Pyr(B, [(H, W)])
    M, hw = pyr.rows, H * W
    x = g(rnd(rng, M, C, scale=2.0), dt)
    bn = make_bn(x, pyr, C, rng)
    gt = g(torch.rand(B, C) + 0.5, "f32") if gate else None
    lz = LazyDesc(x, pyr, C, bn=bn, act=act, gate=gt)
    exact = not act and not gate
    dv = ints(rng, (M, C), -2, 2, dt) if exact else g(rnd(rng, M, C), dt)
    assert not exact or M * 2 < EXACT
    acc_t, acc = bngrad64(1, C)
    L.call("edet_lazy_bwd_reduce", DT[dt], lz.c, pyr.c, C, vp(dv), None, None, acc, stream())
    dxs = []
    for _ in range(2):
        dx = nan_like(M, C, dt)
        L.call("edet_lazy_bwd_apply", DT[dt], lz.c, pyr.c, C, vp(dv), None, None, acc, None, vp(dx), 0, stream())
        dxs.append(dx)
    torch.cuda.synchronize()
    bits = torch.int16 if dt == "bf16" else torch.int32
    assert torch.equal(dxs[0].view(bits), dxs[1].view(bits)), f"{rows}: dx differs between runs"
    su, sq, ga, be = bn_tables(bn)
    cf = BnBwdClosedForm(su, sq, ga, be, M, act=act)
    gc = gt.double().cpu() if gate else None

    def operands(blk):
        d = dv[blk].double().cpu()
        if gate:
            d = d * gc[torch.arange(blk.start, blk.stop) // hw]
        return x[blk].double().cpu(), d

    blocks = row_blocks(0, M)
    for blk in blocks:
        cf.add(*operands(blk))
    if exact:
        assert torch.equal(acc_t[1, 0].cpu(), cf.dbeta), f"{rows}: dbeta max diff {float((acc_t[1, 0].cpu() - cf.dbeta).abs().max())}"
    else:
        close(acc_t[1, 0], cf.dbeta, dt, scale=M ** 0.5 * 2)
    close(acc_t[0, 0], cf.dgamma, dt, scale=M ** 0.5 * 2)
    for blk in blocks:
        close(dxs[0][blk], cf.dx(*operands(blk)), dt)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B,H,W", [(32, 128, 128), (33, 127, 126)])
def test_lazy_materialize_long(dt, B, H, W):
    """M1: gated swish(bn(x)) of 144 channels written out over >= 524288 rows (8-pass chunks)."""
    rng = np.random.default_rng(31 + B)
    C = 144
    pyr = Pyr(B, [(H, W)])
    x = g(rnd(rng, pyr.rows, C), dt)
    lz = LazyDesc(x, pyr, C, bn=make_bn(x, pyr, C, rng), act=1, gate=g(torch.rand(B, C), "f32"))
    outs = []
    for _ in range(2):
        out = nan_like(pyr.rows, C, dt)
        L.call("edet_lazy_materialize", DT[dt], lz.c, pyr.c, C, vp(out), stream())
        outs.append(out)
    torch.cuda.synchronize()
    bits = torch.int16 if dt == "bf16" else torch.int32
    assert torch.equal(outs[0].view(bits), outs[1].view(bits)), "output differs between runs"
    for blk in row_blocks(0, pyr.rows):
        close(outs[0][blk], lz.cpu_rows(blk), dt)


# ----------------------------------------------------------------- depthwise
def img_blocks(B, hw, rows=1 << 18):
    """Image ranges [b0, b1) of about `rows` rows each."""
    step = max(1, rows // hw)
    return [(b0, min(B, b0 + step)) for b0 in range(0, B, step)]


def dw_images(v, n, H, W, k, s, w):
    """fp64 TF-SAME depthwise conv of n images v [n*H*W, C] -> [n*OH*OW, C]; w [k*k, C]."""
    C = v.shape[1]
    xi = v.view(n, H, W, C).permute(0, 3, 1, 2)
    OH, OW = -(-H // s), -(-W // s)
    ph, pw = max((OH - 1) * s + k - H, 0), max((OW - 1) * s + k - W, 0)
    xi = Fn.pad(xi, (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2))
    y = Fn.conv2d(xi, w.t().reshape(C, 1, k, k), stride=s, groups=C)
    return y.permute(0, 2, 3, 1).reshape(-1, C)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("row,s,B,H,W,C,lazy", [("D1", 1, 32, 128, 128, 24, 1), ("D1", 1, 33, 127, 126, 24, 0),
                                                ("D2", 2, 32, 256, 256, 96, 1)])
def test_dwconv_fwd_long(dt, row, s, B, H, W, C, lazy):
    """k3 depthwise forward with BN statistics on the row-streaming form at its 2x (stride 1,
    >= 524288 input rows) and 4x (stride 2, >= 2^21) block targets.  The plain case has x and
    w of {-1, 0, 1}: |y| <= 9 and sum y is exact; sum y^2 on the bar of test_dwconv_fwd_large."""
    rng = np.random.default_rng(s * 10 + C + B)
    k = 3
    pin = Pyr(B, [(H, W)])
    pout = pin.strided(s)
    OH, OW = pout.sizes[0]
    if lazy:
        x = g(rnd(rng, pin.rows, C), dt)
        lz = LazyDesc(x, pin, C, bn=make_bn(x, pin, C, rng), act=1, gate=g(torch.rand(B, C), "f32"))
        w = g(rnd(rng, k * k, C, scale=0.3), dt)
    else:
        x, w = ints(rng, (pin.rows, C), -1, 1, dt), ints(rng, (k * k, C), -1, 1, dt)
        lz = LazyDesc(x, pin, C)
        assert pout.rows * 9 < EXACT
    ys, sts = [], []
    for _ in range(2):
        y, st = nan_like(pout.rows, C, dt), stats_out(1, C)
        names = routed("edet_dwconv_fwd", DT[dt], lz.c, pin.c, C, k, s, vp(w), vp(y), pout.c, stat_out(st), stream())
        assert names == ["k_dws"], (row, names)
        ys.append(y)
        sts.append(st)
    torch.cuda.synchronize()
    bits = torch.int16 if dt == "bf16" else torch.int32
    assert torch.equal(ys[0].view(bits), ys[1].view(bits)), f"{row}: output differs between runs"
    wc = w.double().cpu()
    rs, rq = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    for b0, b1 in img_blocks(B, H * W):
        ref = dw_images(lz.cpu_rows(slice(b0 * H * W, b1 * H * W)), b1 - b0, H, W, k, s, wc)
        close(ys[0][b0 * OH * OW:b1 * OH * OW], ref, dt)
        rs += ref.sum(0)
        rq += (ref * ref).sum(0)
    n = pout.rows
    if lazy:
        close(sts[0][0][0], rs, dt, scale=n ** 0.5 * 4)
    else:
        assert torch.equal(sts[0][0][0].v.cpu(), rs), f"{row}: sum y max diff {float((sts[0][0][0].v.cpu() - rs).abs().max())}"
    close(sts[0][0][1], rq, dt, scale=n ** 0.5 * 8, rtol=5e-2 if dt == "bf16" else 1e-4)


def dw_bwd_images(v, dy, n, H, W, k, s, w):
    """fp64 gradients of sum(dwconv(v) * dy) over n images: (dv [n*H*W, C], dw [k*k, C])."""
    vr, wr = v.clone().requires_grad_(True), w.clone().requires_grad_(True)
    (dw_images(vr, n, H, W, k, s, wr) * dy).sum().backward()
    return vr.grad, wr.grad


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B,H,W", [(32, 128, 128), (33, 127, 126)])
def test_dwconv_bwd_long(dt, B, H, W):
    """D3: the fused stride-1 k3 backward (dx, dW and the folded BN-backward sums of the input)
    of 24 channels over >= 524288 rows: the row-streaming kernel at its 2x block target."""
    rng = np.random.default_rng(24 + B)
    C, k = 24, 3
    pin = Pyr(B, [(H, W)])
    M, hw = pin.rows, H * W
    x = g(rnd(rng, M, C, scale=2.0), dt)
    bn = make_bn(x, pin, C, rng)
    lz = LazyDesc(x, pin, C, bn=bn, act=1)
    w = g(rnd(rng, k * k, C, scale=0.3), dt)
    dy = g(rnd(rng, M, C), dt)
    dxs = []
    for _ in range(2):
        dx, dw = nan_like(M, C, dt), zeros(k * k, C)
        sums_t, sums = bngrad64(1, C)
        names = routed("edet_dwconv_bwd", DT[dt], lz.c, pin.c, C, k, 1, vp(dy), pin.c, vp(w), vp(dx), 0, vp(dw), sums, stream())
        assert names == ["k_dwb"], names
        dxs.append(dx)
    torch.cuda.synchronize()
    bits = torch.int16 if dt == "bf16" else torch.int32
    assert torch.equal(dxs[0].view(bits), dxs[1].view(bits)), "dx differs between runs"
    su, sq, ga, be = bn_tables(bn)
    cf = BnBwdClosedForm(su, sq, ga, be, M, act=1)
    wc = w.double().cpu()
    refw = torch.zeros(k * k, C, dtype=torch.float64)
    for b0, b1 in img_blocks(B, hw):
        sl = slice(b0 * hw, b1 * hw)
        dvr, dwr = dw_bwd_images(lz.cpu_rows(sl), dy[sl].double().cpu(), b1 - b0, H, W, k, 1, wc)
        close(dxs[0][sl], dvr, dt)
        refw += dwr
        cf.add(x[sl].double().cpu(), dvr)
    close(dw, refw, dt, scale=M ** 0.5 * 3)
    close(sums_t[1, 0], cf.dbeta, dt, scale=M ** 0.5 * 2)
    close(sums_t[0, 0], cf.dgamma, dt, scale=M ** 0.5 * 2)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B,sizes,act", [(16, [(256, 256)], 1), (17, [(255, 250)], 0), (16, [(256, 256), (31, 17)], 1)])
def test_dwconv_dgrad_fold_long(dt, B, sizes, act):
    """D4 / D5: the folded k3 s2 k_dw4_dgrad kernel (>= 2^20 input rows) and the plain dgrad
    at the same size, both against fp64: dx, and the fold's sums of the stored dx.  The ragged
    act-free case has dy and w of {-1, 0, 1} (at most 4 taps reach an input pixel at stride 2:
    |dx| <= 4), so the fold's dbeta = sum dx is exact."""
    rng = np.random.default_rng(320 + B + len(sizes))
    C, k, s = 32, 3, 2
    pin = Pyr(B, sizes)
    pout = pin.strided(s)
    nseg = pin.nseg
    x = g(rnd(rng, pin.rows, C, scale=2.0), dt)
    bn = make_bn(x, pin, C, rng)
    lz = LazyDesc(x, pin, C, bn=bn, act=act)
    exact = not act
    if exact:
        dy, w = ints(rng, (pout.rows, C), -1, 1, dt), ints(rng, (k * k, C), -1, 1, dt)
        assert pin.rows * 4 < EXACT
    else:
        dy, w = g(rnd(rng, pout.rows, C), dt), g(rnd(rng, k * k, C, scale=0.3), dt)
    dxs = []
    for _ in range(2):
        dx = nan_like(pin.rows, C, dt)
        acc_t, acc = bngrad64(nseg, C)
        names = routed("edet_dwconv_dgrad_fold", DT[dt], vp(dy), pout.c, C, k, s, vp(w), vp(dx), pin.c, lz.c, acc, stream())
        assert names == ["k_dw4_dgrad"], names  # below 2^20 rows: k_dw4_dgrad, k_lazy_bwd_reduce
        dxs.append(dx)
    dxp = nan_like(pin.rows, C, dt)
    names = routed("edet_dwconv_dgrad", DT[dt], vp(dy), pout.c, C, k, s, vp(w), vp(dxp), pin.c, 0, stream())
    assert names == ["k_dw4_dgrad"], names
    torch.cuda.synchronize()
    bits = torch.int16 if dt == "bf16" else torch.int32
    wc = w.double().cpu()
    for sg in range(nseg):
        H, W = pin.sizes[sg]
        OH, OW = pout.sizes[sg]
        hw, ohw = H * W, OH * OW
        o0, p0 = pin.row_off[sg], pout.row_off[sg]
        ssl = pin.seg_slice(sg)
        assert torch.equal(dxs[0][ssl].view(bits), dxs[1][ssl].view(bits)), f"segment {sg}: dx differs between runs"
        su, sq, ga, be = (t.double().cpu() for t in bn[sg])
        n = pin.seg_rows(sg)
        cf = BnBwdClosedForm(su, sq, ga, be, n, act=act)
        for b0, b1 in img_blocks(B, hw):
            sl = slice(o0 + b0 * hw, o0 + b1 * hw)
            dyb = dy[p0 + b0 * ohw:p0 + b1 * ohw].double().cpu()
            ref, _ = dw_bwd_images(torch.zeros(sl.stop - sl.start, C, dtype=torch.float64), dyb, b1 - b0, H, W, k, s, wc)
            close(dxs[0][sl], ref, dt)
            close(dxp[sl], ref, dt)
            cf.add(x[sl].double().cpu(), dxs[0][sl].double().cpu())  # the fold sums the stored dx
        if exact:
            assert torch.equal(acc_t[1, sg].cpu(), cf.dbeta), f"dbeta max diff {float((acc_t[1, sg].cpu() - cf.dbeta).abs().max())}"
        else:
            close(acc_t[1, sg], cf.dbeta, dt, scale=n ** 0.5)
        close(acc_t[0, sg], cf.dgamma, dt, scale=n ** 0.5)


# ----------------------------------------------------------------- per-image reductions
@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("row,B,HW,C", [("S1", 32, 16384, 144), ("S2", 8, 65536, 16), ("S2", 3, 65536, 32),
                                        ("S2", 5, 129 * 127, 96)])
def test_img_reductions_long(dt, row, B, HW, C):
    """S1-S3: SE squeeze, gate gradient and the SE-fused BN reduce at H*W = 16384 / 65536 (many
    chunks per image; the pass-halving loops end at 16 / 8 / 4 passes), per image against fp64.
    Sums of H*W terms per output: the sqrt(n) * 2 bar the other sum checks use."""
    rng = np.random.default_rng(C + HW + B)
    pyr = Pyr(B, [(HW, 1)])
    x = g(rnd(rng, pyr.rows, C, scale=2.0), dt)
    bn = make_bn(x, pyr, C, rng)
    lz = LazyDesc(x, pyr, C, bn=bn, act=1)
    dv = g(rnd(rng, pyr.rows, C), dt)
    sq, dg, s5 = zeros64(B, C), zeros64(B, C), zeros64(5, B, C)
    L.call("edet_se_squeeze", DT[dt], lz.c, B, HW, C, vp(sq), stream())
    L.call("edet_gate_grad", DT[dt], lz.c, B, HW, C, vp(dv), vp(dg), stream())
    L.call("edet_gate_bn_reduce", DT[dt], lz.c, B, HW, C, vp(dv), vp(s5), stream())
    torch.cuda.synchronize()
    su, sm, ga, be = bn_tables(bn)
    mean = su / pyr.rows
    rstd = 1.0 / torch.sqrt(torch.clamp(sm / pyr.rows - mean * mean, min=0) + 1e-3)
    rsq, r5 = torch.zeros(B, C, dtype=torch.float64), torch.zeros(5, B, C, dtype=torch.float64)
    for n in range(B):
        sl = slice(n * HW, (n + 1) * HW)
        xhat = (x[sl].double().cpu() - mean) * rstd
        u = xhat * ga + be
        d = dv[sl].double().cpu()
        sw, dsw = u * torch.sigmoid(u), dswish(u)
        rsq[n] = sw.mean(0)
        for q, t in enumerate((d * sw, d * dsw, dsw, d * dsw * xhat, dsw * xhat)):
            r5[q, n] = t.sum(0)
    close(sq, rsq, dt)
    close(dg, r5[0], dt, scale=HW ** 0.5 * 2)
    close(s5, r5, dt, scale=HW ** 0.5 * 2)
