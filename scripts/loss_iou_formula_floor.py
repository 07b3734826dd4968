"""Prints the fp32-formula error floor tests/test_loss_iou_gpu.py derives its f32 bar from: its
formulas() (autograd) in fp32 torch against fp64 on the CPU over every level layout, kind and
storage type of its cases.  R: the worst relative deviation over the elements >= 2^-10 of their
level's maximum; F: the worst absolute one over that maximum for the smaller elements.  The fp64
evaluation also asserts that the file's seeds keep every min / max 1e-3 px away from a tie."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_loss_iou_gpu as T  # noqa: E402

if __name__ == "__main__":
    R = F = 0.0
    for sizes in (T.SMALL, T.CHUNKED):
        pyr, box = T.inputs(sizes)[:2]
        for kind in T.KINDS:
            for dt in T.DTS:
                got = T.formulas(sizes, kind, box.to(T.TDT[dt]).float(), torch.float32)[2]
                for s in range(pyr.nseg):
                    g_, r_ = got[pyr.seg_slice(s)], T.reference(sizes, kind, dt)[2][pyr.seg_slice(s)]
                    m, err = float(r_.abs().max()), (g_ - r_).abs()
                    big = r_.abs() >= 2.0 ** -10 * m
                    r, f = float((err[big] / r_.abs()[big]).max()), float(err[~big].max()) / m if (~big).any() else 0.0
                    print(f"{sizes[0][0]:3d}x{sizes[0][1]:<3d} level {s} {kind:5s} {dt:4s} R={r:.3e} F={f:.3e}")
                    R, F = max(R, r), max(F, f)
    print(f"R = {R:.3e}  F = {F:.3e}  (test constants: R {T.R_F32:.3e}, F {T.F_F32:.3e})")
