"""edet_detection_loss_iou (csrc/loss.hip, k_box_iou): Huber + IoU / GIoU / DIoU / CIoU box loss
against fp64 autograd of the definition in include/edet.h, and EfficientDetNetTrain.iou_loss_type.

The comparison is tests/test_loss_gpu.py's: the reference reads the stored (bf16-rounded)
predictions; d loss / d box per level in normalised units (times 4 N+ / box_weight), elementwise
|got - ref| <= rtol * |ref| + floor * max_level |ref|.  scripts/loss_iou_formula_floor.py evaluates
formulas() in fp32 torch on the CPU over every layout, kind and storage type here: R = 6.219e-6, the
worst relative deviation from fp64 over the elements >= 2^-10 of their level's maximum, F = 5.825e-9,
the worst absolute one over that maximum for the smaller elements (both 17x16, ciou, f32).  The
kernel gets 4x that (test_loss_gpu.py's margin and reason); bf16 rtol = 2^-8, the same floor.  Loss
and iou_parts: 1e-4 relative on what the call added.
SEED[sizes]: the first seed (0, 0) with no min / max of the fp64 reference within 1e-3 px of a tie.
"""
import functools
import math

import numpy as np
import pytest
import torch

from tf2mv_amd import _lib as L
from tf2mv_amd.runtime import Pyr, stream, vp
from gpu_util import DEV, DT, TDT, g

pytestmark = pytest.mark.gpu
A, NC, DELTA, BW, WEIGHT, SENT, CLIP = 9, 2, 0.1, 50.0, 0.5, 7.0, math.log(1000.0 / 16.0)
KINDS, DTS, R_F32, F_F32 = list(L.IOU_LOSS), ["f32", "bf16"], 6.219e-6, 5.825e-9  # measured: the module docstring
RTOL, FLOOR = {"f32": 4 * R_F32, "bf16": 2.0 ** -8}, 4 * F_F32
SMALL, CHUNKED = ((3, 2), (1, 1)), ((17, 16), (2, 2))  # CHUNKED: 272 rows, a second LBOX_ROWS chunk of 16
SEED, BATCH = {SMALL: 0, CHUNKED: 0}, {SMALL: 2, CHUNKED: 1}
CASES = [  # ldb: no pad / pad / the scalar fallback; gradient buffer in place / separate / none
    (SMALL, 40, "inplace"), (SMALL, 36, "separate"), (SMALL, 37, "inplace"), (SMALL, 40, "none"),
    (CHUNKED, 40, "inplace"), (CHUNKED, 37, "separate")]


def dn(a, b):  # a / b, and 0 with zero gradient where b == 0
    return torch.where(b != 0, a / torch.where(b != 0, b, torch.ones_like(b)), torch.zeros_like(a))


def iou_loss(p, t, an, kind):
    """L of include/edet.h for p, t, an [..., 4]; the smallest gap between the arguments of a min / max (px)."""
    ha, wa = an[..., 2] - an[..., 0], an[..., 3] - an[..., 1]
    yca, xca = (an[..., 0] + an[..., 2]) / 2, (an[..., 1] + an[..., 3]) / 2
    def dec(r):  # noqa: E306
        h, w = torch.exp(r[..., 2].clamp(-CLIP, CLIP)) * ha, torch.exp(r[..., 3].clamp(-CLIP, CLIP)) * wa
        yc, xc = r[..., 0] * ha + yca, r[..., 1] * wa + xca
        return yc, xc, h, w, yc - h / 2, xc - w / 2, yc + h / 2, xc + w / 2
    (pyc, pxc, ph, pw, *P), (tyc, txc, th, tw, *T) = dec(p), dec(t)
    dy, dx = torch.minimum(P[2], T[2]) - torch.maximum(P[0], T[0]), torch.minimum(P[3], T[3]) - torch.maximum(P[1], T[1])
    inter = dy.clamp(min=0) * dx.clamp(min=0)
    U = ph * pw + th * tw - inter
    loss = 1 - (iou := dn(inter, U))
    ey, ex = torch.maximum(P[2], T[2]) - torch.minimum(P[0], T[0]), torch.maximum(P[3], T[3]) - torch.minimum(P[1], T[1])
    if kind == "giou":
        loss = loss + dn(ey * ex - U, ey * ex)
    if kind in ("diou", "ciou"):
        loss = loss + dn((pyc - tyc) ** 2 + (pxc - txc) ** 2, ey ** 2 + ex ** 2)
    if kind == "ciou":
        v = 4 / math.pi ** 2 * (torch.atan(dn(tw, th)) - torch.atan(dn(pw, ph))) ** 2
        loss = loss + dn(v, 1 - iou + v).detach() * v
    return loss, torch.stack([(P[j] - T[j]).abs() for j in range(4)] + [dy.abs(), dx.abs()]).min(0).values.detach()


@functools.lru_cache(maxsize=None)
def inputs(sizes):
    """pyr, box [rows, A, 4], box_t, mask [rows, A], anchors [N, 4], their per-row gather, N+ - 1, the
    levels' rows, the disjoint positives (ty, tx off by +-3).  Rows between the levels: SENT, mask 1."""
    rng = np.random.default_rng(SEED[sizes])
    pyr = Pyr(BATCH[sizes], list(sizes))
    rows = pyr.rows
    N = lambda *s: torch.tensor(rng.standard_normal(s) * 0.2, dtype=torch.float32)
    bt, box, mask, u = N(rows, A, 4), N(rows, A, 4), torch.tensor(rng.random((rows, A)) < 0.3), torch.tensor(rng.random((rows, A)))
    near, far = mask & (u < 2 / 3), mask & (u >= 2 / 3)
    off = torch.cat([torch.tensor(rng.choice([-3.0, 3.0], (rows, A, 2)), dtype=torch.float32), N(rows, A, 2)], -1)
    box[near], box[far] = (bt + N(rows, A, 4))[near], (bt + off)[far]
    an_rows, flat, valid = torch.zeros(rows, A, 4), [], torch.zeros(rows, dtype=torch.bool)
    for s, (H, W) in enumerate(sizes):
        sl, st = pyr.seg_slice(s), 8.0 * 2 ** s
        valid[sl] = True
        c = (torch.stack(torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij"), -1) + 0.5) * st
        half = torch.tensor(rng.uniform(1.0, 3.0, (H, W, A, 2)), dtype=torch.float32) * st
        lv = torch.cat([c[:, :, None] - half, c[:, :, None] + half], -1)
        flat.append(lv.reshape(-1, 4))
        an_rows[sl] = lv.repeat(pyr.batch, 1, 1, 1).reshape(-1, A, 4)
        r, a = torch.nonzero(near[sl], as_tuple=True)  # th / tw beyond the clamp on the level's first near positives
        for k, j, v in zip(range(len(r)), (2, 3, 2, 3), (5.0, -5.0, -5.0, 5.0)):
            box[sl][r[k], a[k], j] = v
    box[~valid], bt[~valid], mask[~valid] = SENT, SENT, True
    return pyr, box, bt, mask.to(torch.uint8), torch.cat(flat), an_rows, float(mask[valid].sum()), valid, far


def formulas(sizes, kind, stored, dtype):
    """Per level IoU term and Huber term, and d (BW * huber + WEIGHT * iou) / d box [rows, A, 4]."""
    pyr, _, bt, mask, _, an, npos, valid, far = inputs(sizes)
    b, t, pos = stored.to(dtype).clone().requires_grad_(True), bt.to(dtype), valid[:, None] & (mask != 0)
    (loss, gap), e = iou_loss(b, t, an.to(dtype), kind), b - t
    hub = torch.where(e.abs() <= DELTA, 0.5 * e ** 2, 0.5 * DELTA ** 2 + DELTA * (e.abs() - DELTA)) * (t != 0)
    iou_l = [(loss[pyr.seg_slice(s)] * pos[pyr.seg_slice(s)]).sum() / (npos + 1) for s in range(pyr.nseg)]
    hub_l = [hub[pyr.seg_slice(s)].sum() / (4 * (npos + 1)) for s in range(pyr.nseg)]
    (BW * sum(hub_l) + WEIGHT * sum(iou_l)).backward()
    grad = b.grad.double()
    if dtype == torch.float64:
        assert float(gap[pos].min()) > 1e-3, "a min / max of the reference is within 1e-3 px of a tie: next seed"
        if kind == "iou":  # disjoint boxes: Huber's gradient alone, saturated by the +-3 offsets
            assert torch.allclose(grad[far & pos][:, :2].abs() * 4 * (npos + 1) / BW, torch.tensor(DELTA, dtype=dtype))
    return [float(v.detach()) for v in iou_l], [float(v.detach()) for v in hub_l], grad


reference = functools.lru_cache(maxsize=None)(  # fp64, from the values storage type dt holds
    lambda sizes, kind, dt: formulas(sizes, kind, inputs(sizes)[1].to(TDT[dt]).float(), torch.float64))


def run(sizes, ldb, mode, kind, dt, box, bt, mask, iou=True, pre=0.25):
    """One call: what it added to loss, level_parts, iou_parts (pre-loaded with `pre`); dcls, dbox."""
    pyr, anchors, npos, valid = (inputs(sizes)[i] for i in (0, 4, 6, 7))
    rows, ldc, rng = pyr.rows, 24, np.random.default_rng(5)
    box_h = torch.tensor(rng.standard_normal((rows, ldb)), dtype=torch.float32)  # noise in the pad columns
    box_h[:, :A * 4] = box.reshape(rows, -1)
    cls_g, box_g = g(torch.tensor(rng.standard_normal((rows, ldc)), dtype=torch.float32), dt), g(box_h, dt)
    ct, box_0 = torch.tensor(rng.integers(0, NC, (rows, A)), dtype=torch.int32).to(DEV), box_g.clone()
    dc, db = {"inplace": (cls_g, box_g), "none": (None, None),
              "separate": (torch.full_like(cls_g, SENT), torch.full_like(box_g, SENT))}[mode]
    acc = [torch.full((n,), pre, dtype=torch.float32, device=DEV) for n in (1, 2 * L.MAX_SEG, L.MAX_SEG)]
    npos_g, bt_g, mask_g, an_g = torch.tensor([npos], dtype=torch.float32).to(DEV), bt.to(DEV), mask.to(DEV), anchors.to(DEV)
    args = [DT[dt], vp(cls_g), ldc, vp(box_g), ldb, pyr.c, A, NC, vp(ct), vp(bt_g), vp(npos_g), 0.25, 1.5, DELTA, BW, 1.0,
            vp(dc) if dc is not None else None, vp(db) if db is not None else None, vp(acc[0]), vp(acc[1])]
    extra = [vp(an_g), vp(mask_g), L.IOU_LOSS[kind], WEIGHT, vp(acc[2])] if iou else []
    L.call("edet_detection_loss_iou" if iou else "edet_detection_loss", *args, *extra, stream())
    torch.cuda.synchronize()
    assert mode == "inplace" or torch.equal(box_g, box_0)
    if db is not None:  # rows between the levels untouched, pad columns 0
        before = box_0 if mode == "inplace" else torch.full_like(box_0, SENT)
        assert torch.equal(db[~valid.to(DEV)], before[~valid.to(DEV)]) and (db[valid.to(DEV)][:, A * 4:] == 0).all()
    return [a.double().cpu() - pre for a in acc], dc, db


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("sizes,ldb,mode", CASES, ids=lambda v: str(v[0][0]) if isinstance(v, tuple) else str(v))
def test_against_fp64_autograd(sizes, ldb, mode, kind, dt):
    (pyr, box, bt, mask, _, _, npos, _, _), (iou_l, hub_l, ref) = inputs(sizes), reference(sizes, kind, dt)
    (loss, parts, iparts), _, db = run(sizes, ldb, mode, kind, dt, box, bt, mask)
    want, got = BW * sum(hub_l) + WEIGHT * sum(iou_l), float(loss) - float(parts[:L.MAX_SEG].sum())  # less focal
    want_i = torch.tensor(iou_l + [0.0] * (L.MAX_SEG - pyr.nseg), dtype=torch.float64)
    assert abs(got - want) <= 1e-4 * want and ((iparts - want_i).abs() <= 1e-4 * want_i).all(), (got, want, iparts, want_i)
    for s in range(pyr.nseg if db is not None else 0):
        k = 4 * (npos + 1) / BW
        g_, r_ = db.float().cpu()[:, :A * 4].view(-1, A, 4)[pyr.seg_slice(s)].double() * k, ref[pyr.seg_slice(s)] * k
        bad = (g_ - r_).abs() > RTOL[dt] * r_.abs() + FLOOR * r_.abs().max()
        assert not bad.any(), f"level {s}: {int(bad.sum())} over the bar; first got {g_[bad][0]:.9g} ref {r_[bad][0]:.9g}"


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("ldb", [40, 37])
@pytest.mark.parametrize("zero_t", [False, True])
def test_no_positives_equals_plain_loss(zero_t, ldb, dt):
    """All masks 0: dcls and dbox (Huber on the file's non-zero targets) bit for bit edet_detection_loss's,
    iou_parts untouched.  k_box_iou sums a block's n = 4 A rows Huber terms (>= 0) in another order, each
    fp32 sum within n 2^-24 of exact: loss, level_parts to 2 n 2^-24; bit for bit with zero targets."""
    pyr, box, bt, mask = (v * 0 if zero_t and i == 2 else v for i, v in enumerate(inputs(SMALL)[:4]))
    (l0, p0, _), dc0, db0 = run(SMALL, ldb, "inplace", "ciou", dt, box, bt, mask * 0, iou=False, pre=0.0)
    (l1, p1, i1), dc1, db1 = run(SMALL, ldb, "inplace", "ciou", dt, box, bt, mask * 0, pre=0.0)
    bits = lambda t: t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)
    assert torch.equal(bits(dc0), bits(dc1)) and torch.equal(bits(db0), bits(db1)) and (i1 == 0).all()
    tol, live = 0.0 if zero_t else 2 * 4 * A * pyr.rows * 2.0 ** -24, zero_t or (db0.float().abs().sum() > 0 and p0[L.MAX_SEG] > 0)
    assert live and float(l0) > 0 and abs(float(l0 - l1)) <= tol * float(l0) and ((p0 - p1).abs() <= tol * p0.abs()).all()


@pytest.mark.parametrize("kind", KINDS)
def test_perfect_prediction(kind):
    """Predictions equal to the targets on every positive (f32): at most 1e-6 of loss each."""
    _, box, bt, mask, _, _, npos, valid, _ = inputs(SMALL)
    box = torch.where((mask != 0)[..., None], bt, box)
    (_, _, iparts), _, _ = run(SMALL, 40, "none", kind, "f32", box, bt, mask)
    assert float(bt[valid].abs().max()) < CLIP and abs(float(iparts.sum())) * (npos + 1) <= 1e-6 * npos


def test_model_option():
    """test_step adds weight x the fp64 IoU term; compute_step's loss is the sum of its parts; ValueErrors."""
    import test_model_gpu as M
    m, anchors = M._train_model("f32")
    x, boxes, cls, n = M.synth(4)
    (t, yb, yc, ym), xg = M.make_targets(m, anchors, boxes, cls, n), torch.tensor(x).cuda()
    data = (xg, torch.tensor(boxes), torch.tensor(cls), *([torch.tensor(v) for v in y] for y in (yb, yc, ym)))
    base = m.test_step(data)["loss"]
    m.iou_loss_type, m.iou_loss_weight = "diou", 0.5
    got = m.test_step(data)["loss"] - base
    bo, _ = m.call(xg, training=False)
    term = sum(float((iou_loss(bo[s].double().cpu(), torch.tensor(yb[s]).double(), anchors.boxes[s].double().cpu(), "diou")[0]
                      * torch.tensor(ym[s][..., 0])).sum()) for s in range(len(yb))) / (sum(float(v.sum()) for v in ym) + 1)
    assert term > 0 and abs(got - 0.5 * term) <= 1e-4 * term, (got, 0.5 * term)
    m.iou_loss_type = "ciou"
    m.forward_backward((xg, t))
    lp, ip = m.level_parts.double().cpu(), m.iou_parts.double().cpu()
    want = float(lp[:L.MAX_SEG].sum() + 50 * lp[L.MAX_SEG:].sum() + 0.5 * ip.sum())
    assert float(ip.sum()) > 0 and abs(float(m.scalars[0]) - want) <= 1e-4 * want, (float(m.scalars[0]), want)
    assert all(np.isfinite(v).all() for v in m.P.grads_dict().values())
    bare = M.EfficientDetNetTrain(M.efficientnet_b0_blocks(), M.cfg(), None, dtype="f32")
    for model, model.iou_loss_type in ((m, "siou"), (bare, "giou")):
        with pytest.raises(ValueError):
            model.forward_backward((xg, t))
