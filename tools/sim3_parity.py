#!/usr/bin/env python3
"""Writes profiles/sim3_parity.md, on the CPU, from the restatement alone (tests/sim3_ref.py over the scene list of tests/sim3_scene.py): the rules'
s, R, t beside an independent float64 solution of the same triples (numpy.linalg.eigh on N), and rule Z4's rotation beside the reference's
quaternion -> atan2 -> angle-axis -> Rodrigues route evaluated in float64, with the inlier verdicts that differ between the two. tests/test_sim3_cpu.py
repeats both measurements and reads the second from the file this writes.

    python tools/sim3_parity.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sim3_scene as S  # noqa: E402


def main():
    sc = S.scene_list()
    refs = S.ref_run(sc)
    ds, dR, dt = S.measure_float64(sc, refs)
    worst, differ, total = S.measure_angle_axis(sc, refs)
    n_hyp = sum(r["iterations"] for r in refs)
    lines = ["# Sim3 RANSAC: what the rules' arithmetic and rule Z4's deviation change", "",
             "Written by `tools/sim3_parity.py` on the CPU from `tests/sim3_ref.py` over the scene list of `tests/sim3_scene.py`",
             "(%d jobs, %d hypotheses, %d inlier verdicts). `tests/test_sim3_cpu.py` repeats both measurements." % (len(refs), n_hyp, total), "",
             "## The rules beside a float64 solution of the same triples", "",
             "Horn's closed form in float64 throughout, the eigenvector from `numpy.linalg.eigh`; the rules hold float32 wherever the reference holds a",
             "float (Z3). The largest absolute difference over every hypothesis of the scene list:", "",
             "| quantity | largest difference |", "|---|---|",
             "| s | %.3e |" % ds, "| an entry of R | %.3e |" % dR, "| an entry of t | %.3e |" % dt, "",
             "The CPU test allows 4 x these figures; the factor is for other seeds.", "",
             "## Z4 beside the reference's angle-axis route", "",
             "The same float32 quaternion through atan2, the angle-axis vector and Rodrigues' formula in float64, rounded to float32 once, in place of",
             "Z4's direct form; then every hypothesis scored under either rotation:", "",
             "| quantity | value |", "|---|---|",
             "| largest entry difference of R | %.3e |" % worst,
             "| inlier verdicts that differ | %d of %d |" % (differ, total), ""]
    path = os.path.join(ROOT, "profiles", "sim3_parity.md")
    with open(path, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
