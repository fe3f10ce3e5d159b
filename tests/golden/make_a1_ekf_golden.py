"""Generate tests/golden/a1_ekf.npz: 8 robots x 48 ticks of
a1est.synth_inputs through the literal numpy restatement of A1BasicEKF
(tests/a1_est_ref.py): the estimator inputs of every tick, x and the
drift-branch record at every tick, P at four checkpoints.

    python tests/golden/make_a1_ekf_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import a1_est_ref as R  # noqa: E402

OUT = os.path.join(HERE, "a1_ekf.npz")
CHECKPOINTS = (0, 15, 31, 47)


def main():
    inp = R.golden_case()
    X, P, C, TK, MG = R.reference("golden")
    keep = ("dt", "movement_mode", "root_rot_mat", "imu_acc", "imu_ang_vel", "foot_pos_rel",
            "foot_vel_rel", "foot_force")
    np.savez(OUT, **{k: inp[k] for k in keep}, x=X, P=P[list(CHECKPOINTS)],
             checkpoints=np.array(CHECKPOINTS, np.int32), contacts=(C >= 0.5).astype(np.uint8),
             drift_taken=TK, det_margin=MG)
    print(OUT, os.path.getsize(OUT), "bytes; drift taken", int(TK.sum()), "of", TK.size)


if __name__ == "__main__":
    main()
