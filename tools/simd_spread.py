"""Per-SIMD end-time spread of the literal N = 10 kernel at the headline batch
(the tail the one-wave-per-instance launch waits on).

    python tools/simd_spread.py build [map]    (CPU: builds tools/_var/spread/libqloco.so)
    QLOCO_LIB=tools/_var/spread/libqloco.so python tools/simd_spread.py run [B] [GAIT] [shuffle] [noplace]   (GPU)

noplace: the solver without its placement state, workgroup p
solving instance p.  build map: tools/_var/spread_map/libqloco.so, workgroup p
solving order[p] (the placement map alone, before place_assign, §3r).  With
the state the run also prints how the SIMDs' four iteration counts compare
with the assignment's on the same counts.

The variant (tools/variant_lib.py --patch, never the product library) wraps
srbd_lit_kernel: lane 0 of every workgroup reads the 100 MHz real-time
counter before and after the solve and the wave's hardware ids (HW_ID: SIMD
[5:4], CU [11:8], SH [12], SE [15:13]; XCC_ID), and writes them over the
first seven floats of its own u row (vector stores) -- the u output of this
variant is therefore not the solution.  The run aggregates per SIMD: the
first start, the last end, the summed busy time, the number of waves it ran,
and prints the spread of the SIMD end times against the kernel span."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

OLD = """  if (i < 0 || i >= a.batch) return;
  srbd_lit_one<1, WS>(a, S, i);
}"""
NEW = """  if (i < 0 || i >= a.batch) return;
  const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
  srbd_lit_one<1, WS>(a, S, i);
  const uint64_t t1 = __builtin_amdgcn_s_memrealtime();
  const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);
  const unsigned xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);
  if (threadIdx.x == 0 && a.u) {
    unsigned *o = reinterpret_cast<unsigned *>(a.u + i * (12 * a.N));
    o[0] = (unsigned)t0; o[1] = (unsigned)(t0 >> 32);
    o[2] = (unsigned)t1; o[3] = (unsigned)(t1 >> 32);
    o[4] = hw; o[5] = xcc; o[6] = blockIdx.x;
  }
}"""


# the solve kernel's choice of rank (place_assign) against the
# placement map alone (workgroup p solves order[p], §3q)
ASSIGN = "place_position(place_assign(i, a.batch, a.place_simds), a.batch, a.place_simds)"


def build(old_assignment=False):
    import variant_lib
    patches = ["--patch", "qloco_srbd_lit.hip:" + OLD + "=>" + NEW]
    if old_assignment:
        patches += ["--patch", "qloco_srbd_lit.hip:" + ASSIGN + "=>i"]
    variant_lib.main(["spread_map" if old_assignment else "spread"] + patches)


def run(B, gait, shuffle=False, placement=True):
    import torch

    from quadrupedal_loco_amd import _lib, srbd
    if os.environ.get("QLOCO_LIB"):
        _lib.LIB_PATH = os.environ["QLOCO_LIB"]
    N = 10
    dev = torch.device("cuda:0")
    x0, xr, ft, ct = srbd.generate(20261015, N, B, gait)
    if shuffle:  # bench.py's shuffled_order line: the same seeded permutation
        perm = np.random.default_rng(20261015 + 1).permutation(B)
        x0, xr, ft, ct = (a[perm] for a in (x0, xr, ft, ct))
    args = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (x0, xr, ft, ct)]
    s = srbd.BatchedConvexMpc(horizon=N, literal_full_qp=1, placement=placement)
    out = s.alloc_outputs(B, dev, full=True)
    for _ in range(60):  # past the clock ramp
        s.solve(*args, out=out, max_legs=4 * N)
    torch.cuda.synchronize()
    reps = []
    for _ in range(5):
        s.solve(*args, out=out, max_legs=4 * N)
        torch.cuda.synchronize()
        reps.append(out.u.view(torch.int32).cpu().numpy().reshape(B, 12 * N)[:, :7].astype(np.uint32))
    it = out.iters.cpu().numpy()
    for r, w in enumerate(reps):
        t0 = w[:, 0].astype(np.uint64) | (w[:, 1].astype(np.uint64) << np.uint64(32))
        t1 = w[:, 2].astype(np.uint64) | (w[:, 3].astype(np.uint64) << np.uint64(32))
        hw, xcc = w[:, 4], w[:, 5] & 0xF
        wg = w[:, 6].astype(np.int64)  # the workgroup that solved the instance
        simd = (hw >> 4) & 3
        cu = (hw >> 8) & 0xF
        sh = (hw >> 12) & 1
        se = (hw >> 13) & 7
        key = (((xcc.astype(np.int64) * 8 + se) * 2 + sh) * 16 + cu) * 4 + simd
        base = t0.min()
        s0 = (t0 - base).astype(np.float64) * 0.01  # 100 MHz ticks -> us
        s1 = (t1 - base).astype(np.float64) * 0.01
        span = s1.max()
        keys, inv = np.unique(key, return_inverse=True)
        end = np.zeros(len(keys))
        busy = np.zeros(len(keys))
        nw = np.zeros(len(keys), int)
        itsum = np.zeros(len(keys))
        np.maximum.at(end, inv, s1)
        np.add.at(busy, inv, s1 - s0)
        np.add.at(nw, inv, 1)
        np.add.at(itsum, inv, it)
        pct = np.percentile(end, [0, 10, 50, 90, 100])
        print("rep %d: B=%d %s%s%s  kernel span %.1f us  SIMDs used %d (XCCs %d)  waves/SIMD min %d max %d" % (
            r, B, gait, " shuffled" if shuffle else "", "" if placement else " unplaced", span, len(keys), len(np.unique(xcc)), nw.min(), nw.max()))
        print("   SIMD end time us: min %.1f p10 %.1f p50 %.1f p90 %.1f max %.1f;  mean SIMD idle tail %.1f us "
              "(%.1f%% of the span)" % (*pct, span - end.mean(), 100 * (span - end.mean()) / span))
        print("   per-wave solve us: p50 %.1f p99 %.1f max %.1f;  per-SIMD iterations sum min %d p50 %d max %d" % (
            *np.percentile(s1 - s0, [50, 99, 100]), itsum.min(), np.median(itsum), itsum.max()))
        if r == 0:
            # dispatch placement: do the workgroups sharing a SIMD follow p mod (number of SIMDs)?
            nsimd = len(keys)
            same = np.mean([len(set((wg[inv == k] % nsimd).tolist())) == 1 for k in range(nsimd)])
            print("   placement: %.3f of SIMDs hold workgroups with one value of p mod %d; "
                  "SIMD key of workgroups 0..7: %s" % (same, nsimd, key[np.argsort(wg)[:8]].tolist()))
            if placement and nsimd < B <= 4 * nsimd and hasattr(_lib.lib(), "qloco_srbd_place_assign_host"):
                # the four counts of every SIMD against place_assign's on these counts
                # (as multisets of sorted tuples: the order inside a class is the atomics')
                import collections
                import lit_placement_model as M
                want = M._per_simd(it, M.assigned_order(it, nsimd), nsimd).astype(int)
                got = np.zeros((nsimd, 4), int)
                for k in range(nsimd):
                    c = np.sort(it[inv == k])[-4:]
                    got[k, 4 - len(c):] = c
                cw = collections.Counter(map(tuple, want))
                cg = collections.Counter(map(tuple, got))
                print("   assignment: %d of %d SIMDs hold the counts place_assign gives; modelled span %.1f us" % (
                    sum((cw & cg).values()), nsimd, M.simd_us(it, M.assigned_order(it, nsimd), nsimd).max()))
            late = np.argsort(-end)[:3]
            for k in late:
                sel = inv == k
                print("   late SIMD key %d: %d waves, iterations %s, end %.1f us" % (
                    keys[k], nw[k], sorted(it[sel].tolist()), end[k]))
        sys.stdout.flush()


if __name__ == "__main__":
    if sys.argv[1] == "build":
        build("map" in sys.argv[2:])
    else:
        run(int(sys.argv[2]) if len(sys.argv) > 2 else 4096, sys.argv[3] if len(sys.argv) > 3 else "trot",
            "shuffle" in sys.argv[4:], "noplace" not in sys.argv[4:])
