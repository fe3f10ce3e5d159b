"""Generate tests/golden/a1_kin_ref.npz: A1 leg kinematics vectors computed
with the REFERENCE's own arithmetic.

A1Kinematics.cpp needs Eigen to compile as a unit; its computing part is the
two generated closed forms autoFunc_fk_derive / autoFunc_d_fk_dq
(unitree_ros/a1_cpp_open_source/src/legKinematics/A1Kinematics.cpp:39-130),
plain C in q, rho_opt and rho_fix.  This script reads the two function bodies
out of the reference file at generation time, places them in a throwaway C
harness in a temporary directory and evaluates them with gcc (-O2
-ffp-contract=off, x86-64 double).  Nothing of the reference is stored in the
repository: the committed fixture holds only inputs and outputs.

    python tests/golden/make_a1_kin_golden.py <path to A1Kinematics.cpp>   # needs gcc

Rows: the four stand-pose known answers (legs FL, FR, RL, RR), then 400
random rows with leg = row % 4, so every four rows are one robot.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "a1_kin_ref.npz")
# GazeboA1ROS.cpp:79-101
RHO_FIX = np.array([[0.1805, 0.047, 0.0838, 0.21, 0.21], [0.1805, -0.047, -0.0838, 0.21, 0.21],
                    [-0.1805, 0.047, 0.0838, 0.21, 0.21], [-0.1805, -0.047, -0.0838, 0.21, 0.21]])
STAND_Q = (0.0, 0.72, -1.44)


def _body(src, name):
    i = src.index("void A1Kinematics::" + name)
    i = src.index("{", i)
    depth, j = 0, i
    while True:
        depth += {"{": 1, "}": -1}.get(src[j], 0)
        j += 1
        if depth == 0:
            return src[i:j].replace("std::", "")


def _harness(fk, jac):
    return "\n".join([
        "#include <math.h>", "#include <stdio.h>",
        "static void fk(const double in1[3], const double in2[3], const double in3[5], double p_bf[3])",
        fk,
        "static void jac(const double in1[3], const double in2[3], const double in3[5], double jacobian[9])",
        jac,
        "int main(void) {",
        "  double q[3], v[3], ro[3] = {0.0, 0.0, 0.0}, rf[5], p[3], J[9];",
        "  while (scanf(\"%lf %lf %lf %lf %lf %lf %lf %lf %lf %lf %lf\", q, q + 1, q + 2, v, v + 1, v + 2,",
        "               rf, rf + 1, rf + 2, rf + 3, rf + 4) == 11) {",
        "    fk(q, ro, rf, p); jac(q, ro, rf, J);",
        "    for (int r = 0; r < 3; r++) printf(\"%a \", p[r]);",
        "    for (int r = 0; r < 9; r++) printf(\"%a \", J[r]);",
        "    for (int r = 0; r < 3; r++) printf(\"%a \", J[r] * v[0] + J[3 + r] * v[1] + J[6 + r] * v[2]);",
        "    printf(\"\\n\");",
        "  }",
        "  return 0;", "}"]) + "\n"


def main(ref):
    src = open(ref).read()
    rng = np.random.default_rng(20261019)
    leg, q, qd = [], [], []
    for l in range(4):
        leg.append(l)
        q.append(np.array(STAND_Q))
        qd.append(np.zeros(3))
    for k in range(400):
        leg.append(k % 4)
        q.append(np.array([rng.uniform(-0.8, 0.8), rng.uniform(-1.0, 2.5), rng.uniform(-2.7, -0.9)]))
        qd.append(rng.uniform(-8.0, 8.0, 3))
    lines = [" ".join("%r" % float(v) for v in (*q[k], *qd[k], *RHO_FIX[leg[k]])) for k in range(len(leg))]
    with tempfile.TemporaryDirectory() as td:
        c, exe = os.path.join(td, "h.c"), os.path.join(td, "h")
        open(c, "w").write(_harness(_body(src, "autoFunc_fk_derive"), _body(src, "autoFunc_d_fk_dq")))
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", c, "-lm", "-o", exe], check=True)
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True,
                             check=True).stdout
    vals = np.array([[float.fromhex(t) for t in ln.split()] for ln in out.splitlines() if ln.strip()])
    assert vals.shape == (len(leg), 15)
    np.savez(OUT, leg=np.array(leg, np.int32), q=np.array(q), qd=np.array(qd),
             pos=vals[:, 0:3], jac=vals[:, 3:12], vel=vals[:, 12:15])
    print(OUT, len(leg), "rows; stand-pose feet", vals[:4, 0:3].tolist())


if __name__ == "__main__":
    main(sys.argv[1])
