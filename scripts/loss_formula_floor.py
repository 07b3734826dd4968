"""Prints the fp32-formula error floor that tests/test_loss_gpu.py derives its f32 bar from: the
textbook focal + Huber formulas evaluated in fp32 torch against fp64 on the CPU, over every case
of that file (R: worst relative deviation, F: worst absolute one over the level maximum)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_loss_gpu as T  # noqa: E402

if __name__ == "__main__":
    R, F = T.measure_fp32_formula(lambda c, dt, r, f: print(f"{str(c):50s} {dt:4s} R={r:.3e} F={f:.3e}"))
    print(f"R = {R:.3e}  F = {F:.3e}  (test constants: R {T.R_F32:.3e}, F {T.F_F32:.3e})")
