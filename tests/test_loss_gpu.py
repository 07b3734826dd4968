"""Detection loss (csrc/loss.hip): every route of k_loss against one fp64 reference, in units in
which a wrong factor shows; edet_count_positives and edet_onehot_to_index exactly.

Routes of k_loss's class part (all three launch the same kernel; the arguments select):
  (a) packed pairs (focal_pair15): gamma == 1.5, NC >= 8, ldc % 8 == 0, bf16, dcls == cls
  (b) 8-wide vectors: ldc % 8 == 0 and dcls null or == cls, whenever (a) does not apply
      (f32 storage; bf16 with NC < 8, gamma != 1.5 or dcls null)
  (c) scalar: ldc % 8 != 0, or dcls a separate buffer
The box part (Huber) is one route, in LBOX_ROWS chunks.

The comparison.  The reference reads the *stored* logits and box predictions (the bf16
roundings for bf16 storage), so only the kernel's own error is left.  Gradients are compared
per level in normalised units: d loss/d logit times N+ * rows_l * A * NC * count_scale and
d loss/d box times 4 N+ / box_weight are O(1) at every level size.  Elementwise
    |got - ref| <= rtol * |ref| + floor * max_level |ref|.

The constants.  `python scripts/loss_formula_floor.py` (measure_fp32_formula below) evaluates the same textbook formulas (autograd)
in plain fp32 torch on the CPU for every case of this file, both storage types, and reports
their worst deviation from the fp64 reference in these units: R, the worst relative deviation
over the elements with |ref| >= 2^-10 of their level's maximum, and F, the worst absolute
deviation over the level's maximum for the smaller elements (a saturated easy negative is
1e-20 of its neighbours and cannot be held to a relative bar).  Measured (torch 2.x CPU):
    R = 1.430e-6 (NC = 8, levels 3x2 and 1x1, bf16 values),  F = 1.457e-9 (NC = 5, gamma = 1, f32)
The kernel gets 4x that: it uses 1-ulp hardware exp / log / rsq / rcp where torch rounds
correctly, and it reassociates:
    f32:   rtol = 4 R = 5.7e-6,  floor = 4 F = 5.8e-9
    bf16:  rtol = 2^-8 (rounding to bf16's 8 significant bits moves a value by at most
           2^-8 / (1 + 2^-8) of itself; the 1.5e-5 left below 2^-8 is for the fp32 arithmetic
           ahead of the store, which the f32 bar holds to 5.7e-6),  floor = 4 F (the arithmetic
           is fp32 for both storage types)
The loss scalar and level_parts are fp32 sums in both storage types: rtol 1e-4 of the reference
value, measured on what the call added to the pre-loaded accumulators.
"""
import dataclasses
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from tf2mv_amd import _lib as L
from tf2mv_amd.runtime import Pyr, stream, vp
from gpu_util import DEV, DT, TDT, g

pytestmark = pytest.mark.gpu
DTS = ["f32", "bf16"]
A = 9
MAX_SEG = L.MAX_SEG
SENT = 7.0  # rows between the levels and untouched gradient buffers

R_F32, F_F32 = 1.430e-6, 1.457e-9  # measured: see the module docstring
RTOL = {"f32": 4 * R_F32, "bf16": 2.0 ** -8}
FLOOR = 4 * F_F32
SPLIT = 2.0 ** -10  # elements below SPLIT * level max are measured against the floor
SCALAR_RTOL = 1e-4
SPECIAL = [0.0] + [s * v for v in (2.0 ** -10, 15.0, 40.0, 88.0, 200.0) for s in (1.0, -1.0)]


def roundup8(n):
    return (n + 7) // 8 * 8


@dataclasses.dataclass(frozen=True)
class Case:
    NC: int
    sizes: tuple
    ldc: int = 0          # 0: roundup8(A * NC)
    ldb: int = 40
    B: int = 2
    alpha: float = 0.25
    gamma: float = 1.5
    delta: float = 0.1
    bw: float = 50.0
    cs: float = 1.0
    kind: str = "noise"   # noise | special | targets | nopos
    mode: str = "inplace"  # inplace | none | separate  (the gradient buffers)
    seed: int = 0

    @property
    def ld(self):
        return self.ldc or roundup8(A * self.NC)

    def data(self):
        """The case with the fields that do not change inputs or reference reset: the key the
        inputs and references are shared under (ldc only adds pad columns)."""
        return dataclasses.replace(self, mode="inplace", ldc=0, ldb=40)

    def __str__(self):
        d = Case(self.NC, self.sizes)
        diff = [f"{f.name}={getattr(self, f.name)}" for f in dataclasses.fields(self)[2:]
                if getattr(self, f.name) != getattr(d, f.name)]
        return f"NC{self.NC}-" + "x".join(f"{h}.{w}" for h, w in self.sizes) + "".join("-" + s for s in diff)


CASES = []  # every case of this file (the fp32-formula measurement walks them)


def cases(*cs):
    CASES.extend(cs)
    return pytest.mark.parametrize("c", cs, ids=str)


# ------------------------------------------------------------------ inputs and references
@functools.lru_cache(maxsize=None)
def logical(d: Case):
    """Unrounded fp32 inputs of a case without pad columns: cls [rows, A*NC], box [rows, A*4],
    ct [rows, A] int32, bt [rows, A, 4], npos_sum."""
    rng = np.random.default_rng(1000 + d.seed + d.NC)
    pyr = Pyr(d.B, list(d.sizes))
    NC, rows = d.NC, pyr.rows
    cls = torch.tensor(rng.standard_normal((rows, A * NC)) * 3.0, dtype=torch.float32)
    box = torch.tensor(rng.standard_normal((rows, A * 4)) * 0.2, dtype=torch.float32)
    ct = torch.tensor(rng.integers(0, NC, (rows, A)), dtype=torch.int32)
    bt = torch.tensor(rng.standard_normal((rows, A, 4)) * 0.2, dtype=torch.float32)
    bt[torch.tensor(rng.random((rows, A, 4)) < 0.5)] = 0.0
    if d.kind == "nopos":
        ct[:] = 0
        bt[:] = 0.0
    if d.kind == "targets":
        u = torch.tensor(rng.random((rows, A)))
        ct[u < 0.15] = -1          # no positive column (tf.one_hot of an out-of-range index)
        ct[u > 0.85] = NC
        u = torch.tensor(rng.random((rows, A, 4)))
        bv = box.view(rows, A, 4)
        bv[u < 0.1], bt[u < 0.1] = 0.25, 0.375    # pred - t == -delta (delta = 0.125)
        bv[u > 0.9], bt[u > 0.9] = 0.5, 0.375     # pred - t == +delta
    if d.kind == "special":
        assert NC >= 2
        cv = cls.view(rows, A, NC)
        for s in range(pyr.nseg):
            r0 = pyr.row_off[s]
            assert pyr.seg_rows(s) * A >= len(SPECIAL)
            for i, v in enumerate(SPECIAL):  # anchor i of the level: its positive class and class 0
                r, a, k = r0 + i // A, i % A, 1 + i % (NC - 1)
                ct[r, a] = k
                cv[r, a, k] = v
                cv[r, a, 0] = v
    valid = torch.zeros(rows, dtype=torch.bool)
    for s in range(pyr.nseg):
        valid[pyr.seg_slice(s)] = True
    cls[~valid], box[~valid] = SENT, SENT
    npos = float(((ct > 0) & (ct < NC))[valid].sum())
    return pyr, cls, box, ct, bt, npos


def stored(d: Case, dt):
    """What the device buffers hold for storage type dt (values, fp32)."""
    _, cls, box, _, _, _ = logical(d)
    return cls.to(TDT[dt]).float(), box.to(TDT[dt]).float()


def loss_formulas(d: Case, cls, box, dtype):
    """Sigmoid focal + Huber detection loss and its gradients by the textbook formulas in
    `dtype`, from the stored values cls [rows, A*NC] / box [rows, A*4].  The class target is
    built by comparison, so an index outside [0, NC) gives an all-zero row (as tf.one_hot).
    Returns total, per-level focal terms, per-level box terms (without box_weight), dcls, dbox."""
    pyr, _, _, ct, bt, npos = logical(d)
    NC = d.NC
    npr = npos + 1.0
    xs = cls.to(dtype).clone().requires_grad_(True)
    bs = box.to(dtype).clone().requires_grad_(True)
    tot, focal, boxl = 0.0, [], []
    for s in range(pyr.nseg):
        sl = pyr.seg_slice(s)
        x = xs[sl].view(-1, A, NC)
        y = (ct[sl].long()[..., None] == torch.arange(NC)).to(dtype)
        p = torch.sigmoid(x)
        pt = y * p + (1 - y) * (1 - p)
        at = y * d.alpha + (1 - y) * (1 - d.alpha)
        # sigmoid cross entropy max(x, 0) - x y + log(1 + exp(-|x|)), written through logsigmoid(x) =
        # min(x, 0) - log1p(exp(-|x|)): the same arithmetic, but autograd gives it the derivative
        # sigmoid(x) - y at x == 0 too, where max and |.| take a one-sided one
        ce = -(y * Fn.logsigmoid(x) + (1 - y) * Fn.logsigmoid(-x))
        f = (at * (1 - pt) ** d.gamma * ce).sum() / (npr * x.numel() * d.cs)
        t = bt[sl].to(dtype).view(-1, A * 4)
        e = bs[sl] - t
        hub = torch.where(e.abs() <= d.delta, 0.5 * e ** 2, 0.5 * d.delta ** 2 + d.delta * (e.abs() - d.delta))
        b = (hub * (t != 0)).sum() / (4 * npr)
        tot = tot + d.bw * b + f
        focal.append(float(f.detach()))
        boxl.append(float(b.detach()))
    tot.backward()
    return float(tot.detach()), focal, boxl, xs.grad.double(), bs.grad.double()


@functools.lru_cache(maxsize=None)
def reference(d: Case, dt):
    cls, box = stored(d, dt)
    return loss_formulas(d, cls, box, torch.float64)


def level_scales(d: Case):
    """Per level: the factors that bring dcls and dbox to O(1) units."""
    pyr, _, _, _, _, npos = logical(d)
    return [((npos + 1.0) * pyr.seg_rows(s) * A * d.NC * d.cs, 4.0 * (npos + 1.0) / d.bw) for s in range(pyr.nseg)]


def deviation(d: Case, got_c, got_b, dt):
    """[(what, level, R, F)] of got against the fp64 reference in normalised units: R the worst
    relative deviation over the elements >= SPLIT * level max, F the worst absolute deviation
    over the level max for the others."""
    pyr = logical(d)[0]
    _, _, _, rc, rb = reference(d, dt)
    out = []
    for s, (kc, kb) in enumerate(level_scales(d)):
        sl = pyr.seg_slice(s)
        for what, got, ref, k in (("dcls", got_c, rc, kc), ("dbox", got_b, rb, kb)):
            if got is None:
                continue
            g_, r_ = got[sl].double() * k, ref[sl] * k
            m = float(r_.abs().max())
            err = (g_ - r_).abs()
            big = r_.abs() >= SPLIT * m
            rel = float((err[big] / r_.abs()[big]).max()) if m > 0 and big.any() else 0.0
            if m > 0:
                fl = float(err[~big].max()) / m if (~big).any() else 0.0
            else:  # an all-zero reference (no positives: dbox): any deviation counts
                fl = float(err.max())
            out.append((what, s, rel, fl))
    return out


def measure_fp32_formula(report=None):
    """R and F of the module docstring: the fp32 evaluation of the reference formulas against
    the fp64 one over every case of this file (CPU only; scripts/loss_formula_floor.py prints
    them).  report(case, dt, R, F) is called per case."""
    R = F = 0.0
    for c in sorted({c.data() for c in CASES}, key=str):
        for dt in DTS:
            cls, box = stored(c, dt)
            _, _, _, gc, gb = loss_formulas(c, cls, box, torch.float32)
            dev = deviation(c, gc, gb, dt)
            r, f = max(v[2] for v in dev), max(v[3] for v in dev)
            if report:
                report(c, dt, r, f)
            R, F = max(R, r), max(F, f)
    return R, F


# ------------------------------------------------------------------ the call
def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@dataclasses.dataclass
class Result:
    loss: float            # what the call added to the accumulators
    focal: list
    boxl: list
    dcls: torch.Tensor     # [rows, A*NC] fp32 values on the host, or None
    dbox: torch.Tensor
    raw_dcls: torch.Tensor  # the storage-type gradient buffer [rows, ldc] on the host, or None


def run(c: Case, dt):
    """One edet_detection_loss call with every structural check: accumulation into pre-loaded
    loss / level_parts, zero pad columns, untouched rows between the levels, untouched inputs
    where the gradient goes elsewhere, scalars against fp64."""
    d = c.data()
    pyr, cls, box, ct, bt, npos = logical(d)
    ref_tot, ref_f, ref_b, _, _ = reference(d, dt)
    NC, AN, A4, ldc, ldb, rows = c.NC, A * c.NC, A * 4, c.ld, c.ldb, pyr.rows
    prng = np.random.default_rng(77)  # pad columns of the inputs hold noise: the gradient's are 0
    cls_h = torch.tensor(prng.standard_normal((rows, ldc)), dtype=torch.float32)
    box_h = torch.tensor(prng.standard_normal((rows, ldb)), dtype=torch.float32)
    cls_h[:, :AN], box_h[:, :A4] = cls, box
    valid = torch.zeros(rows, dtype=torch.bool)
    for s in range(pyr.nseg):
        valid[pyr.seg_slice(s)] = True
    cls_h[~valid], box_h[~valid] = SENT, SENT
    cls_g, box_g = g(cls_h, dt), g(box_h, dt)
    cls_0, box_0 = cls_g.clone(), box_g.clone()
    # the reference was fed exactly what the kernel reads
    cs_, bs_ = stored(d, dt)
    assert torch.equal(cls_0.float().cpu()[:, :AN], cs_) and torch.equal(box_0.float().cpu()[:, :A4], bs_)
    if c.mode == "inplace":
        dc, db = cls_g, box_g
    elif c.mode == "separate":
        dc, db = torch.full_like(cls_g, SENT), torch.full_like(box_g, SENT)
    else:
        dc = db = None
    # accumulators pre-loaded with a quarter of what is to come (2^-12 where that is 0)
    pre = lambda v: float(np.float32(0.25 * v)) if v != 0 else 2.0 ** -12
    loss0 = pre(ref_tot)
    parts0 = [2.0 ** -12] * (2 * MAX_SEG)
    for s in range(pyr.nseg):
        parts0[s], parts0[MAX_SEG + s] = pre(ref_f[s]), pre(ref_b[s])
    loss = torch.tensor([loss0], dtype=torch.float32, device=DEV)
    parts = torch.tensor(parts0, dtype=torch.float32, device=DEV)
    npos_g = torch.tensor([npos], dtype=torch.float32, device=DEV)
    ct_g, bt_g = ct.to(DEV), bt.to(DEV)
    L.call("edet_detection_loss", DT[dt], vp(cls_g), ldc, vp(box_g), ldb, pyr.c, A, NC,
           vp(ct_g), vp(bt_g), vp(npos_g), c.alpha, c.gamma, c.delta, c.bw, c.cs,
           vp(dc) if dc is not None else None, vp(db) if db is not None else None, vp(loss), vp(parts), stream())
    torch.cuda.synchronize()
    got_loss = float(loss.double().cpu()) - loss0
    got_parts = (parts.double().cpu() - torch.tensor(parts0, dtype=torch.float64)).tolist()
    assert math.isfinite(got_loss)
    assert abs(got_loss - ref_tot) <= SCALAR_RTOL * abs(ref_tot), (got_loss, ref_tot)
    for s in range(2 * MAX_SEG):
        lvl = s % MAX_SEG
        want = 0.0 if lvl >= pyr.nseg else (ref_f[lvl] if s < MAX_SEG else ref_b[lvl])
        assert abs(got_parts[s] - want) <= SCALAR_RTOL * abs(want), (s, got_parts[s], want)
    if c.mode != "inplace":  # the inputs are only read
        assert torch.equal(bits(cls_g), bits(cls_0)) and torch.equal(bits(box_g), bits(box_0))
    if dc is None:
        return Result(got_loss, got_parts[:pyr.nseg], got_parts[MAX_SEG:MAX_SEG + pyr.nseg], None, None, None)
    before_c, before_b = (cls_0, box_0) if c.mode == "inplace" else (torch.full_like(cls_g, SENT), torch.full_like(box_g, SENT))
    inv = (~valid).to(DEV)
    assert torch.equal(bits(dc)[inv], bits(before_c)[inv]) and torch.equal(bits(db)[inv], bits(before_b)[inv])
    dch, dbh = dc.cpu(), db.cpu()
    assert torch.isfinite(dch[valid].float()).all() and torch.isfinite(dbh[valid].float()).all()
    assert (dch[valid][:, AN:] == 0).all() and (dbh[valid][:, A4:] == 0).all()
    return Result(got_loss, got_parts[:pyr.nseg], got_parts[MAX_SEG:MAX_SEG + pyr.nseg],
                  dch[:, :AN].float(), dbh[:, :A4].float(), dch)


def check(c: Case, dt):
    """run() and the gradients against the fp64 reference at the module's bar."""
    d = c.data()
    res = run(c, dt)
    if res.dcls is None:
        return res
    pyr = logical(d)[0]
    _, _, _, rc, rb = reference(d, dt)
    for s, (kc, kb) in enumerate(level_scales(d)):
        sl = pyr.seg_slice(s)
        for what, got, ref, k in (("dcls", res.dcls, rc, kc), ("dbox", res.dbox, rb, kb)):
            g_, r_ = got[sl].double() * k, ref[sl] * k
            bar = RTOL[dt] * r_.abs() + FLOOR * r_.abs().max()
            bad = (g_ - r_).abs() > bar
            assert not bad.any(), (f"{what} level {s}: {int(bad.sum())} elements over the bar; first "
                                   f"got {g_[bad][0]:.9g} ref {r_[bad][0]:.9g}; (what, level, R, F) "
                                   f"{deviation(d, res.dcls, res.dbox, dt)} against rtol {RTOL[dt]:.3e} floor {FLOOR:.3e}")
    return res


# ------------------------------------------------------------------ cases
SMALL = ((3, 2), (1, 1))
# gamma = 1.5 throughout.
# NC = 8, ldc = 72 in place: (a) for bf16, (b) for f32;  none: (b) for both;  separate: (c);
# ldc = 76 in place: (c)
ROUTES = [Case(8, SMALL), Case(8, SMALL, mode="none"), Case(8, SMALL, mode="separate"), Case(8, SMALL, ldc=76)]
# NC = 5 (< 8, so never (a)), ldc = 48 in place: (b) for both types, focal_elem15 with the tr[a]
# lookup;  none: (b);  separate: (c);  ldc = 52 in place: (c), focal_elem with g15
ROUTES5 = [Case(5, SMALL), Case(5, SMALL, mode="none"), Case(5, SMALL, mode="separate"), Case(5, SMALL, ldc=52)]


@pytest.mark.parametrize("dt", DTS)
@cases(*ROUTES, *ROUTES5)
def test_routes(c, dt):
    check(c, dt)


def bf16_ulp(v):
    _, e = torch.frexp(v)
    return torch.ldexp(torch.ones_like(v), e - 8)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("routes", [ROUTES, ROUTES5], ids=["NC8", "NC5"])
def test_routes_agree(routes, dt):
    """The four variants of a route matrix against each other on the same data: the losses
    within the scalar bar; the bf16 gradients written in place at ldc % 8 == 0, through a
    separate buffer (c) and at ldc % 8 != 0 (c) within one bf16 ulp.  The in-place one is route
    (a) at NC = 8 and route (b) at NC = 5, so each of the packed, the 8-wide and the scalar
    closed forms stands beside another."""
    res = [run(c, dt) for c in routes]
    for r in res[1:]:
        assert abs(r.loss - res[0].loss) <= SCALAR_RTOL * abs(res[0].loss), (r.loss, res[0].loss)
    if dt == "bf16":
        valid = res[0].dcls[:, 0] != SENT
        for r in (res[2], res[3]):
            for x, y in ((res[0].dcls, r.dcls), (res[0].dbox, r.dbox)):
                x, y = x[valid], y[valid]
                assert ((x - y).abs() <= bf16_ulp(torch.maximum(x.abs(), y.abs()))).all()


@pytest.mark.parametrize("dt", DTS)
@cases(*[Case(NC, ((3, 2),)) for NC in (2, 5, 7, 8, 9, 13, 20, 81, 90, 91)])
def test_nc_sweep(c, dt):
    """The (cv + 0.5) / NC anchor lookup, a vector over two anchors (NC = 8, 9), tr[a] for NC < 8."""
    check(c, dt)


@pytest.mark.parametrize("dt", DTS)
@cases(Case(8, ((2, 2),)), Case(232, ((2, 2),)))
def test_long_rows(c, dt):
    """NC = 232: ldc = 2088, 261 vectors a row, more than the block's 256 threads."""
    check(c, dt)


@pytest.mark.parametrize("dt", DTS)
@cases(Case(8, ((13, 11), (1, 1))))
def test_chunking(c, dt):
    """286 rows in level 0: a second LBOX_ROWS chunk, and a last class chunk of 30 rows."""
    check(c, dt)


@pytest.mark.parametrize("dt", DTS)
@cases(Case(8, SMALL, ldc=88, ldb=48), Case(5, SMALL, ldc=64))
def test_whole_pad_vectors(c, dt):
    """Rows that end in a vector of pad columns only (its anchor index is >= A)."""
    check(c, dt)


@pytest.mark.parametrize("dt", DTS)
@cases(*[Case(NC, SMALL, gamma=gm, mode=m) for gm in (2.0, 1.0) for NC in (8, 5) for m in ("inplace", "none", "separate")])
def test_gamma(c, dt):
    """focal_elem's log / exp branch on routes (b) and (c); gamma = 1.5 on (c) is in test_routes."""
    check(c, dt)


@pytest.mark.parametrize("dt", DTS)
@cases(*[Case(NC, SMALL, gamma=gm, mode=m, kind="special")
         for NC, gm, m in ((8, 1.5, "inplace"), (8, 1.5, "separate"), (5, 1.5, "inplace"), (8, 2.0, "inplace"),
                           (8, 2.0, "separate"), (8, 1.0, "inplace"), (8, 1.0, "separate"))])
def test_saturated_logits(c, dt):
    """0, +-2^-10, +-15, +-40, +-88, +-200 at a positive and at a negative class of every level:
    finite loss and gradients (run()), the same bar."""
    check(c, dt)


@pytest.mark.parametrize("dt", DTS)
@cases(Case(8, SMALL, kind="targets", delta=0.125), Case(8, SMALL, kind="targets", delta=0.125, mode="separate"),
       Case(5, SMALL, kind="targets", delta=0.125))
def test_targets(c, dt):
    """Class targets -1 and NC (no positive column), box targets 0 (masked out), |pred - t| == delta."""
    pyr, _, box, ct, bt, _ = logical(c.data())
    v = pyr.seg_slice(0)
    assert (ct[v] == -1).any() and (ct[v] == c.NC).any()
    assert ((box[v].view(-1, A, 4) - bt[v]).abs() == c.delta).any() and (bt[v] == 0).any()
    check(c, dt)


@pytest.mark.parametrize("dt", DTS)
@cases(Case(8, SMALL, kind="nopos"), Case(8, SMALL, kind="nopos", mode="separate"))
def test_no_positives(c, dt):
    """N+ = 1: the box terms and dbox are exactly 0, the focal part follows fp64."""
    assert logical(c.data())[5] == 0.0
    res = check(c, dt)
    assert res.boxl == [0.0] * len(c.sizes)
    valid = res.dcls[:, 0] != SENT
    assert (res.dbox[valid] == 0).all()


@pytest.mark.parametrize("dt", DTS)
@cases(Case(8, SMALL, cs=2.0), Case(8, SMALL, cs=2.0, mode="separate"))
def test_count_scale(c, dt):
    """focal_count_scale = 2 against fp64 with that scale, and against the call with scale 1: the
    focal terms halve, dcls halves exactly (a power of two), the box terms and dbox do not move."""
    two = check(c, dt)
    one = run(dataclasses.replace(c, cs=1.0), dt)
    valid = one.dcls[:, 0] != SENT
    assert torch.equal(two.dcls[valid] * 2, one.dcls[valid]) and torch.equal(two.dbox[valid], one.dbox[valid])
    for s in range(len(c.sizes)):
        assert abs(2 * two.focal[s] - one.focal[s]) <= 2 * SCALAR_RTOL * abs(one.focal[s])
        assert abs(two.boxl[s] - one.boxl[s]) <= 2 * SCALAR_RTOL * abs(one.boxl[s])


# ------------------------------------------------------------------ count_positives / onehot_to_index
@pytest.mark.parametrize("off", [0, 16])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 65541, 2113543])
def test_count_positives(n, off):
    """Exact count of the non-zero mask bytes, added to `out`.  2113543 = 128 blocks x 1024
    vectors x 16 bytes + 1024 vectors + 7 bytes: a second four-vector trip at the block cap and a
    ragged tail."""
    rng = np.random.default_rng(n + off)
    buf = torch.tensor(rng.choice(np.array([0, 1, 2, 255], dtype=np.uint8), size=off + n))
    buf_g = buf.to(DEV)
    m = buf_g[off:]
    assert m.data_ptr() % 16 == 0
    out = torch.full((1,), 5.0, dtype=torch.float32, device=DEV)
    L.call("edet_count_positives", vp(m), n, vp(out), stream())
    assert float(out.cpu()) == 5.0 + int((buf[off:] != 0).sum())


@pytest.mark.parametrize("NC", [1, 5, 81])
def test_onehot_to_index(NC):
    """The first maximum of each row, as numpy.argmax.  An all-zero row gives 0: the documented
    difference from the inverse of tf.one_hot, which has no index for such a row."""
    n = 1000
    rng = np.random.default_rng(NC)
    oh = np.zeros((n, NC), dtype=np.float32)
    idx = rng.integers(0, NC, n)
    oh[np.arange(n), idx] = 1.0                    # proper one-hot rows
    oh[::7] = 0.0                                  # all-zero rows
    oh[5::7] = rng.standard_normal((len(oh[5::7]), NC)).astype(np.float32)  # any values
    for r in range(3, n, 7) if NC > 1 else ():     # two equal maxima: the first one counts
        oh[r] = 0.0
        oh[r, rng.choice(NC, 2, replace=False)] = 1.0
    assert (oh[::7] == 0).all() and (NC == 1 or ((oh[3::7] == 1).sum(1) == 2).all())
    out = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    oh_g = torch.tensor(oh).to(DEV)
    L.call("edet_onehot_to_index", vp(oh_g), n, NC, vp(out), stream())
    assert np.array_equal(out.cpu().numpy(), np.argmax(oh, axis=1))
