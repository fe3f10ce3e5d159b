"""QP input families for the Goldfarb-Idnani tests, their closed forms and
the oracle wrapper (TEST INFRASTRUCTURE ONLY).

Shared by tests/test_oracle.py, which asserts each family's preconditions
against the restatement alone (oracle/eiquadprog.c: status census, pinned
iteration counts, closed-form error), and tests/test_qp_gpu.py, which runs
the same inputs through qloco_eiquadprog_solve.  A problem is the tuple
(G, g0, CE, ce0, CI, ci0) of numpy arrays, G (n, n), CE (n, p), CI (n, m).

  A  random_feasible_qp  feasible Gaussian QPs (the active set works)
  B  box_qp              diagonal G, box constraints, x = clip(-g0/diag G)
  C  tie_qp              dyadic data, exact ties in the most-violated scan
  D  mixed_status_batch  NOT_PD / infeasible / active-set / slack, cycled
  E  equality_qp         equalities only, KKT closed form
"""
import ctypes as C
import functools
import zlib

import numpy as np

import oracle_lib as O

OK, INFEASIBLE, NOT_PD, DEGENERATE = 0, 2, 5, 6  # qloco_status


def random_qp(rng, n, p, m, zero_ce=0):
    M = rng.standard_normal((n, n))
    G = M @ M.T + n * np.eye(n)
    g0 = rng.standard_normal(n) * 3
    CE = rng.standard_normal((n, p))
    for k in range(min(zero_ce, p)):
        CE[:, rng.integers(p)] = 0.0
    ce0 = rng.standard_normal(p) * 0.3
    CI = rng.standard_normal((n, m))
    ci0 = rng.standard_normal(m) + 0.5
    return G, g0, CE, ce0, CI, ci0


def random_feasible_qp(rng, n, p, m, zero_ce=0):
    """Random QP feasible by construction: equalities and inequalities hold
    at a random point x_f (inequalities strictly), so the solve ends OK and
    exercises the active set (the unconstrained minimum violates many rows)."""
    G, g0, CE, ce0, CI, ci0 = random_qp(rng, n, p, m, zero_ce)
    x_f = rng.standard_normal(n) * 0.3
    ce0 = -CE.T @ x_f
    ci0 = -CI.T @ x_f + np.abs(rng.standard_normal(m)) + 0.1
    return G, g0 * 10, CE, ce0, CI, ci0


def oracle_eqp(G, g0, CE, ce0, CI, ci0):
    n, p, m = G.shape[0], CE.shape[1], CI.shape[1]
    ws = O.lib().qo_eqp_create(n, p, m)
    Gc = np.asfortranarray(G).ravel(order="F").copy()
    CEc = np.asfortranarray(CE).ravel(order="F").copy() if p else np.zeros(1)
    CIc = np.asfortranarray(CI).ravel(order="F").copy() if m else np.zeros(1)
    x = np.zeros(n)
    st, it = C.c_int(0), C.c_int(0)
    ce0c = np.ascontiguousarray(ce0) if p else np.zeros(1)
    ci0c = np.ascontiguousarray(ci0) if m else np.zeros(1)
    f = O.lib().qo_eqp_solve(ws, O.P(Gc), O.P(np.ascontiguousarray(g0)), O.P(CEc), O.P(ce0c),
                             O.P(CIc), O.P(ci0c), O.P(x), C.byref(st), C.byref(it))
    O.lib().qo_eqp_destroy(ws)
    return x, f, st.value, it.value


class Solved:
    """The restatement's results over a list of problems (computed once)."""

    def __init__(self, probs):
        res = [oracle_eqp(*pr) for pr in probs]
        self.x = np.stack([r[0] for r in res])
        self.f = np.array([r[1] for r in res])
        self.status = np.array([r[2] for r in res], np.int32)
        self.iters = np.array([r[3] for r in res], np.int32)

    def census(self):
        return {int(s): int(np.sum(self.status == s)) for s in np.unique(self.status)}

    def iters_crc(self):
        return zlib.crc32(self.iters.astype("<i4").tobytes())


def stack(probs, k):
    """Operand k of every problem, column-major flattened: (B, size)."""
    return np.stack([np.asfortranarray(pr[k]).ravel(order="F") for pr in probs])


def shape_seed(family, *shape):
    return [ord(family)] + [int(v) for v in shape]


# ---- A. feasible Gaussian
FAMILY_A = [(8, 0, 48, 0), (12, 3, 24, 0), (16, 4, 64, 2), (16, 0, 64, 0)]


@functools.lru_cache(maxsize=None)
def family_a(n, p, m, zero_ce, B=64):
    rng = np.random.default_rng(shape_seed("A", n, p, m, zero_ce))
    probs = [random_feasible_qp(rng, n, p, m, zero_ce) for _ in range(B)]
    return probs, Solved(probs)


# ---- B. box, closed form
FAMILY_B = [1, 4, 16, 17, 32, 64]
# max |x - clip(-g0 / diag G, lo, hi)| of the restatement over family_b(n),
# measured (8.88e-16, 2.66e-15, 3.11e-15, 1.78e-15, 2.22e-15, 2.78e-15) and
# rounded up to one digit.  Only the CPU precondition test uses it (the
# restatement stays this close to the closed form); the GPU test bounds the
# kernels by 16x the restatement's error computed on the run's own inputs
BOX_ERR = {1: 9e-16, 4: 3e-15, 16: 4e-15, 17: 2e-15, 32: 3e-15, 64: 3e-15}


def box_qp(rng, n):
    """G = diag(2^k), k in -1..2; lo <= x <= hi as CI = [I, -I], ci0 = (-lo, hi).
    Returns the problem and x = clip(-g0 / diag G, lo, hi) in float64 (one
    division and two compares per entry: correctly rounded)."""
    dg = 2.0 ** rng.integers(-1, 3, n)
    g0 = 6.0 * rng.standard_normal(n)
    lo = -rng.uniform(0.5, 1.5, n)
    hi = rng.uniform(0.5, 1.5, n)
    CI = np.concatenate([np.eye(n), -np.eye(n)], axis=1)
    ci0 = np.concatenate([-lo, hi])
    prob = (np.diag(dg), g0, np.zeros((n, 0)), np.zeros(0), CI, ci0)
    return prob, np.clip(-g0 / dg, lo, hi)


@functools.lru_cache(maxsize=None)
def family_b(n, B=64):
    rng = np.random.default_rng(shape_seed("B", n))
    both = [box_qp(rng, n) for _ in range(B)]
    probs = [b[0] for b in both]
    return probs, Solved(probs), np.stack([b[1] for b in both])


# ---- C. coupled ties
FAMILY_C = [(4, 8), (8, 24), (16, 64), (17, 65), (32, 96)]


def tie_qp(rng, n, m):
    """Dyadic data: G = diag(2^k), k in -1..1, unconstrained minimum x0 in
    {+-4, +-8}^n, CI columns of 2 or 3 entries +-1 (one when n < 3), ci0 in
    {1, 2}: s(x0) takes few distinct values, so the most-violated scan meets
    exact ties.  x = 0 is strictly feasible."""
    dg = 2.0 ** rng.integers(-1, 2, n)
    x0 = rng.choice([-8.0, -4.0, 4.0, 8.0], n)
    CI = np.zeros((n, m))
    for i in range(m):
        k = 1 if n < 3 else int(rng.integers(2, 4))
        CI[rng.choice(n, k, replace=False), i] = rng.choice([-1.0, 1.0], k)
    ci0 = rng.integers(1, 3, m).astype(np.float64)
    return np.diag(dg), -dg * x0, np.zeros((n, 0)), np.zeros(0), CI, ci0


@functools.lru_cache(maxsize=None)
def family_c(n, m, B=64):
    rng = np.random.default_rng(shape_seed("C", n, m))
    probs = [tie_qp(rng, n, m) for _ in range(B)]
    return probs, Solved(probs)


# ---- D. mixed statuses in one wave
FAMILY_D = (8, 0, 24)
FAMILY_D_BATCH = 67
FAMILY_D_KINDS = ("not_pd", "infeasible", "active", "slack")


def mixed_status_qp(rng, kind, n=8, m=24):
    G, g0, CE, ce0, CI, ci0 = random_feasible_qp(rng, n, 0, m)
    if kind == "not_pd":  # one negative diagonal entry: Cholesky stops there
        G = G.copy()
        k = int(rng.integers(n))
        G[k, k] = -G[k, k]
    elif kind == "infeasible":  # c'x >= 1 + b and -c'x >= 1 - b
        i, j = rng.choice(m, 2, replace=False)
        CI[:, j] = -CI[:, i]
        b = rng.standard_normal()
        ci0[i], ci0[j] = -1.0 - b, -1.0 + b
    elif kind == "slack":  # every constraint slack at the unconstrained minimum
        xu = -np.linalg.solve(G, g0)
        ci0 = -CI.T @ xu + 1.0 + np.abs(rng.standard_normal(m))
    return G, g0, CE, ce0, CI, ci0


@functools.lru_cache(maxsize=None)
def family_d(B=FAMILY_D_BATCH):
    n, _, m = FAMILY_D
    rng = np.random.default_rng(shape_seed("D", n, m))
    probs = [mixed_status_qp(rng, FAMILY_D_KINDS[b % 4], n, m) for b in range(B)]
    return probs, Solved(probs)


# ---- E. equality only
FAMILY_E = [(16, 16), (4, 2), (20, 17)]
# max |x - x_kkt| / max(1, |x_kkt|max) of the restatement over family_e(n, p),
# measured (7.86e-14, 5.07e-16, 8.15e-15; p = n = 16 is a square Gaussian
# solve, |x| up to 95) and rounded up to the decade, since the inputs go
# through the platform's BLAS.  Only the CPU precondition test uses it; the
# GPU test bounds the kernels by 16x the restatement's error computed on
# the run's own inputs
KKT_ERR = {(16, 16): 1e-13, (4, 2): 1e-15, (20, 17): 1e-14}


def equality_qp(rng, n, p):
    """Gaussian full-rank CE (p <= n), no inequalities.  Returns the problem
    and the KKT solution [G CE; CE' 0] [x; lam] = [-g0; -ce0] by numpy in
    float64 with one refinement step on an np.longdouble residual."""
    G, g0, CE, ce0, _, _ = random_qp(rng, n, p, 0)
    K = np.block([[G, CE], [CE.T, np.zeros((p, p))]])
    rhs = np.concatenate([-g0, -ce0])
    sol = np.linalg.solve(K, rhs)
    res = rhs.astype(np.longdouble) - K.astype(np.longdouble) @ sol.astype(np.longdouble)
    sol = sol + np.linalg.solve(K, res.astype(np.float64))
    return (G, g0, CE, ce0, np.zeros((n, 0)), np.zeros(0)), sol[:n]


@functools.lru_cache(maxsize=None)
def family_e(n, p, B=64):
    rng = np.random.default_rng(shape_seed("E", n, p))
    both = [equality_qp(rng, n, p) for _ in range(B)]
    probs = [b[0] for b in both]
    return probs, Solved(probs), np.stack([b[1] for b in both])


# ---- more live equality columns than variables
OVERFULL = [(2, 3, 0), (4, 6, 4), (20, 24, 8)]


@functools.lru_cache(maxsize=None)
def overfull(n, p, m, B=8):
    rng = np.random.default_rng(shape_seed("O", n, p, m))
    probs = [random_qp(rng, n, p, m) for _ in range(B)]
    return probs, Solved(probs)


# ---- edge shapes and the shapes one step past each dispatch limit
EDGES = [(1, 0, 0, 0), (1, 0, 2, 0), (1, 1, 0, 0), (16, 0, 0, 0), (16, 16, 64, 2),
         (17, 0, 8, 0), (4, 0, 65, 0), (20, 17, 8, 0)]


@functools.lru_cache(maxsize=None)
def edge(n, p, m, zero_ce, B=64):
    if (n, p, m) == (1, 0, 2):
        probs, sol, _ = family_b(1, B)
        return probs, sol
    rng = np.random.default_rng(shape_seed("X", n, p, m, zero_ce))
    probs = [random_feasible_qp(rng, n, p, m, zero_ce) for _ in range(B)]
    return probs, Solved(probs)
