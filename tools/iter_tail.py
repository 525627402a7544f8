#!/usr/bin/env python3
"""iter_tail.py — how full the machine is while nn_grid_iter2_kernel runs, from its waves' own clocks.

Needs the diagnostic build of the library (never the default):

    make -C iterative-closest-point_amd OUT=build_dbg EXTRA=-DICP_ITER2_DBG=1 build_dbg/libicp_hip.so
    ICP_AMD_LIB=iterative-closest-point_amd/build_dbg/libicp_hip.so python tools/iter_tail.py [--points N] [--out FILE]

In that build every wave of the fused grid iteration records its entry and exit time (two
s_memrealtime reads, 100 MHz), its strand, its XCD (blockIdx.x & 7) and its walker count; with
ICP_ITER_DEBUG=2 and ICP_ITER_TAIL_DUMP=<file> icp_run appends each launch's records to the file
(icp_run.hip, dump_wave_records).  This tool runs one registration (C4 by default: bench.py's
pair and 30 iterations) after a warm-up one, and reduces the second one's launches to

  * resident waves against time, for each XCD (ten samples a launch),
  * the slot-time left empty between the first wave's exit and the last wave's exit, as a share
    of the launch's slot-time (slots: 256 CUs x 4 SIMDs x 4 waves, 512 an XCD),
  * the rank correlation (Spearman) of each strand's walker count with the launch before.

ICP_ITER2_ORDER picks the dispatch order as in any run (0: xcd_row).
"""
import argparse
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAGIC = 0x4C494154524554
SLOTS_XCD = 512
TICK_US = 0.01


def read_dump(path):
    """[(iteration, n, t0, t1, strand, xcd, walkers)] of the launches in the file"""
    a = np.fromfile(path, dtype=np.uint64)
    out, i = [], 0
    while i + 4 <= len(a):
        assert int(a[i]) == MAGIC, "not an ICP_ITER_TAIL_DUMP file"
        it, nb, n = int(a[i + 1]), int(a[i + 2]), int(a[i + 3])
        rec = a[i + 4:i + 4 + 4 * nb].reshape(nb, 4)
        i += 4 + 4 * nb
        t0, t1, w = rec[:, 0].astype(np.int64), rec[:, 1].astype(np.int64), rec[:, 2]
        out.append((it, n, t0, t1, (w >> np.uint64(32)).astype(np.int64),
                    ((w >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.int64), (w & np.uint64(0xFFFF)).astype(np.int64)))
    return out


def ranks(v):
    """average ranks (ties share their mean rank)"""
    order = np.argsort(v, kind="stable")
    sv = v[order]
    first = np.r_[True, sv[1:] != sv[:-1]]
    start = np.flatnonzero(first)
    end = np.r_[start[1:], len(v)]
    mean = (start + end - 1) / 2.0
    r = np.empty(len(v))
    r[order] = np.repeat(mean, end - start)
    return r


def spearman(a, b):
    ra, rb = ranks(a), ranks(b)
    ra -= ra.mean()
    rb -= rb.mean()
    d = np.sqrt((ra * ra).sum() * (rb * rb).sum())
    return float((ra * rb).sum() / d) if d > 0 else float("nan")


def reduce_launch(t0, t1, xcd):
    """length (ticks), empty share after the first exit (all, per XCD), resident curve [xcd][10]"""
    lo, hi = t0.min(), t1.max()
    length = max(int(hi - lo), 1)
    first_exit = t1.min()

    def empty(sel, slots):
        busy = np.clip(np.minimum(t1[sel], hi) - np.maximum(t0[sel], first_exit), 0, None).sum()
        return (slots * (hi - first_exit) - busy) / float(slots * length)

    xs = sorted(set(xcd.tolist()))
    per = {k: empty(xcd == k, SLOTS_XCD) for k in xs}
    tot = empty(np.ones(len(t0), bool), SLOTS_XCD * len(xs))
    at = lo + (np.arange(10) + 0.5) * length / 10.0
    curve = {k: [int(((t0[xcd == k] <= t) & (t1[xcd == k] > t)).sum()) for t in at] for k in xs}
    return length, tot, per, curve, int(hi - first_exit)


def report(launches, out):
    prev = None
    tots, lens, rhos, drains = [], [], [], []
    for it, n, t0, t1, strand, xcd, walk in launches:
        length, tot, per, curve, after = reduce_launch(t0, t1, xcd)
        by_strand = np.zeros(strand.max() + 1, dtype=np.int64)
        by_strand[strand] = walk
        rho = spearman(prev, by_strand) if prev is not None and len(prev) == len(by_strand) else float("nan")
        prev = by_strand
        # the drain: from the last wave's entry (the block list ran out) to the last exit
        drain = int(t1.max() - t0.max())
        tots.append(tot)
        lens.append(length)
        rhos.append(rho)
        drains.append(drain)
        out.write(f"launch it {it:2d}  n {n}  waves {len(t0)}  length {length * TICK_US:6.2f} us  walkers {int(walk.sum()):7d}"
                  f"  drain after the last entry {drain * TICK_US:5.2f} us  empty after the first exit {100 * tot:5.2f}%"
                  f"  walker rank correlation with the launch before {rho:6.3f}\n")
        out.write("   empty by XCD (%): " + " ".join(f"{100 * per[k]:5.2f}" for k in sorted(per)) + "\n")
        for k in sorted(curve):
            out.write(f"   XCD {k} resident at 5%..95%: " + " ".join(f"{c:3d}" for c in curve[k]) + "\n")
    if launches:
        out.write(f"\nmean of {len(launches)} launches: length {np.mean(lens) * TICK_US:.2f} us, drain after the last entry "
                  f"{np.mean(drains) * TICK_US:.2f} us, empty after the first exit {100 * np.mean(tots):.2f}% of the "
                  f"slot-time, walker rank correlation {np.nanmean(rhos):.3f} (launches with a predecessor)\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default="-")
    ap.add_argument("--dump", help="reduce this dump file instead of running")
    args = ap.parse_args()
    if args.dump:
        launches = read_dump(args.dump)
    else:
        fd, path = tempfile.mkstemp(suffix=".itertail")
        os.close(fd)
        os.environ["ICP_ITER_DEBUG"] = "2"
        os.environ["ICP_ITER_TAIL_DUMP"] = path
        sys.path.insert(0, os.path.join(ROOT, "iterative-closest-point_amd"))
        import icp_amd
        m, p = icp_amd.synthetic_pair(args.points, seed=42)
        with icp_amd.Context(0, icp_amd.NN_CERTIFIED) as ctx:
            for _ in range(2):  # (the first registration warms up; the second one's launches are kept)
                open(path, "wb").close()
                ctx.set_model(m)
                ctx.set_scene(p)
                ctx.run(args.iters, -1.0)
        launches = read_dump(path)
        os.unlink(path)
        if not launches:
            sys.exit("no wave records: the library is not the diagnostic build (-DICP_ITER2_DBG=1), or no fused launch ran")
    out = sys.stdout if args.out == "-" else open(args.out, "w")
    out.write(f"iter_tail: ICP_ITER2_ORDER={os.environ.get('ICP_ITER2_ORDER', '(default)')}  {len(launches)} fused launches\n")
    report(launches, out)


if __name__ == "__main__":
    main()
