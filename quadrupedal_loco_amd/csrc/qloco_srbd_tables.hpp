// qloco_srbd_tables.hpp -- the literal QP's G^-1 horizon tables on the host
// (qloco_srbd_tables.cpp).  Plain C++: included by the host
// translation unit and by the HIP launch path.
#pragma once

namespace qloco {

// The six N x N blocks A_a^-1 of G^-1 (qloco_srbd_lit.hip, "G^-1 in six
// N x N blocks") for a spec whose omega weights are isotropic
// (q2[6] == q2[7]): then the eigenvalues of the omega x / y pair do not
// depend on the yaw, and the tables are a function of (N, dt, q2) alone.
// gtab: NT * NT * 6 floats in LitLds::gtab's layout -- (row step, column
// step, axis) in column-space order, NT = 10 for N <= 10 and 20 above (two
// waves: step r of the second half H = ceil(N / 2) sits at 10 + r - H), zero
// on the padding steps.  sq = 1 / sqrt(q_omega) (S = Rz' / sqrt(q_omega)),
// gmx = max diag G^-1.  Returns false, writing nothing, where the kernel has
// to build the tables per instance (q2[6] != q2[7]) or N is out of range.
bool srbd_lit_tables_host(int N, float dt, const float *q2, float *gtab, float *sq, float *gmx);

// The one-wave tables (N <= 10, 600 floats) through a small spec-keyed host
// cache: a controller keeps its weights, N and dt from call to call, so the
// inverses run once.  Safe from several host threads.
bool srbd_lit_tables_cached(int N, float dt, const float *q2, float *gtab, float *sq, float *gmx);

}  // namespace qloco
