"""Generate tests/golden/a1_ctrl_filter.npz and a1_ctrl_bezier.npz: the two
parts of the A1 gait / swing controller that can be pinned to the REFERENCE's
own arithmetic.

  MovingWindowFilter      utils/filter.hpp is self-contained C++; the harness
                          includes it as it is from the reference directory.
  BezierUtils::bezier_curve  the function body is read out of utils/Utils.cpp
                          (:100-107) at generation time and placed in a
                          throwaway harness (bezier_degree is the float 4 of
                          Utils.h).

Both harnesses live in a temporary directory and are compiled with g++ (-O2
-ffp-contract=off, x86-64 double, glibc pow).  Nothing of the reference is
stored in the repository: the committed fixtures hold only inputs and outputs.

    python tests/golden/make_a1_ctrl_golden.py <path to a1_cpp_open_source/src/utils>   # needs g++

Filter sequences (each longer than both windows, 60 and 100): magnitudes over
six decades with sign changes, so both branches of the Neumaier update are
taken many times (counted by tests/test_a1_ctrl.py on the restatement), a foot
position like stream and a small-angle stream.  Bezier: t over float32 steps
of 1/120 from 0 to 1 (the spline times of the default gait) plus float32
neighbours of 0, 0.5 and 1, for six control polygons of the {s, s, f, f, f}
shape, with and without the z clearance.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

FILTER_MAIN = r"""
#include <cmath>
#include <cstdio>
#include "filter.hpp"
int main() {
  int w, n;
  while (std::scanf("%d %d", &w, &n) == 2) {
    MovingWindowFilter f(w);
    for (int k = 0; k < n; ++k) {
      double v;
      if (std::scanf("%la", &v) != 1) return 1;
      std::printf("%a\n", f.CalculateAverage(v));
    }
  }
  return 0;
}
"""


def _body(src, head):
    i = src.index(head)
    i = src.index("{", i)
    depth, j = 0, i
    while True:
        depth += {"{": 1, "}": -1}.get(src[j], 0)
        j += 1
        if depth == 0:
            return src[i:j]


def _bezier_main(body):
    return "\n".join([
        "#include <cmath>", "#include <cstdio>", "#include <vector>",
        "static float bezier_degree = 4;",
        "static double bezier_curve(double t, const std::vector<double> &P)", body,
        "int main() {",
        "  float t; double p[5];",
        "  while (std::scanf(\"%a %la %la %la %la %la\", &t, p, p + 1, p + 2, p + 3, p + 4) == 6) {",
        "    std::vector<double> P(p, p + 5);",
        "    std::printf(\"%a\\n\", bezier_curve(t, P));",
        "  }", "  return 0;", "}"]) + "\n"


def _run(td, name, text, stdin, inc=None):
    cpp, exe = os.path.join(td, name + ".cpp"), os.path.join(td, name)
    open(cpp, "w").write(text)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off"] + (["-I" + inc] if inc else []) +
                   [cpp, "-o", exe], check=True)
    out = subprocess.run([exe], input=stdin, capture_output=True, text=True, check=True).stdout
    return np.array([float.fromhex(t) for t in out.split()])


def filter_inputs():
    rng = np.random.default_rng(20261019)
    n = 400
    wide = rng.normal(0, 1, (2, n)) * 10.0 ** rng.uniform(-3, 3, (2, n))
    foot = 0.18 + 0.02 * np.sin(np.arange(n) * 0.07) + rng.normal(0, 1e-3, n)
    angle = np.abs(rng.normal(0, 1e-4, n)) + 0.05 * (np.arange(n) > 150)
    return [(60, wide[0]), (100, wide[1]), (60, foot), (100, angle), (60, -foot), (100, foot)]


def bezier_inputs():
    rng = np.random.default_rng(20261020)
    t = [np.float32(k) / np.float32(120.0) for k in range(121)]
    for c in (0.0, 0.5, 1.0):
        c = np.float32(c)
        t += [np.nextafter(c, np.float32(2)), np.nextafter(c, np.float32(-1))]
    t = np.array(t, np.float32)
    polys = []
    for k in range(6):
        s, f = rng.normal(0, 0.3), rng.normal(0, 0.3)
        P = [s, s, f, f, f]
        if k % 2:
            P[1] += float(np.float32(0.0))
            P[2] += float(np.float32(0.4)) + 0.5 * 0.0
        polys.append(P)
    polys.append([0.0, 0.0, 0.0, 0.0, 0.0])
    polys.append([-0.35, -0.35, -0.35 + float(np.float32(0.4)), -0.35, -0.35])
    return t, np.array(polys)


def main(utils_dir):
    src = open(os.path.join(utils_dir, "Utils.cpp")).read()
    with tempfile.TemporaryDirectory() as td:
        seqs = filter_inputs()
        stdin = "".join("%d %d\n%s\n" % (w, len(v), " ".join(float(x).hex() for x in v)) for w, v in seqs)
        avg = _run(td, "filt", FILTER_MAIN, stdin, inc=utils_dir)
        t, polys = bezier_inputs()
        lines = ["%s %s" % (float(tt).hex(), " ".join(float(x).hex() for x in P)) for P in polys for tt in t]
        y = _run(td, "bez", _bezier_main(_body(src, "double BezierUtils::bezier_curve")), "\n".join(lines) + "\n")
    n = len(seqs[0][1])
    assert avg.shape == (len(seqs) * n,) and y.shape == (len(polys) * len(t),)
    np.savez(os.path.join(HERE, "a1_ctrl_filter.npz"), window=np.array([w for w, _ in seqs], np.int32),
             values=np.array([v for _, v in seqs]), average=avg.reshape(len(seqs), n))
    np.savez(os.path.join(HERE, "a1_ctrl_bezier.npz"), t=t, P=polys, y=y.reshape(len(polys), len(t)))
    print("filter", avg.reshape(len(seqs), n)[:, -1], "bezier", y.reshape(len(polys), len(t))[:, 60])


if __name__ == "__main__":
    main(sys.argv[1])
