"""MPI_Reduce_scatter and MPI_Ireduce_scatter through the engine at a sweep of message sizes: a
multi-process rehearsal (the ranks are processes sharing one GPU, so no xGMI byte is timed).

fp32 SUM, equal counts, not in place, 64 KiB .. 256 MiB per rank (the whole vector) in powers of 16.
Legs, each timed the same way -- rank 0's wall time around the call (the nonblocking ones: post +
wait), after a barrier, one call at a time; median, minimum and 90th percentile:
  rs       mi355x_reduce_scatter, the blocking call
  irs0     mi355x_ireduce_scatter + wait under NB_ORDER = 0 (coll/tuned's order: the blocking call's work
           behind the progress-thread hand-off)
  irs1     the same under NB_ORDER = 1 (coll/libnbc's order: never the resident service)
  ar, iar  mi355x_allreduce and mi355x_iallreduce + wait (NB_ORDER = 0): the yardstick for the hand-off
A library without mi355x_ireduce_scatter (an earlier commit: copy this file into its tools/) runs
rs, ar and iar.  Inputs are small integers, so every sum is exact in fp32 whatever the order, and
each leg's result is checked on the device.

usage: python tools/irs_bench.py --n 4 [--label TEXT] [--out FILE] [--legs rs,irs0,irs1,ar,iar]
       (starts the ranks itself; each rank is `python tools/irs_bench.py --rank R --key K ...`)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import uuid

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [64 << 10, 1 << 20, 16 << 20, 256 << 20]
LEGS = ["rs", "irs0", "irs1", "ar", "iar"]


def rank_main(a):
    import torch
    sys.path.insert(0, os.path.dirname(HERE))
    import bench
    pkg = bench.load_pkg()
    pkg.rt()
    rank, n = a.rank, a.n
    torch.cuda.set_device(0)
    comm = pkg.Comm.create(a.key, rank, n, 0)
    comm.set("TIMEOUT_S", 120)
    op, ty = pkg.OP["SUM"], pkg.T["FLOAT"]
    legs = [leg for leg in a.legs.split(",") if leg in LEGS and (hasattr(comm, "ireduce_scatter") or not leg.startswith("irs"))]
    rows = []
    for nbytes in [s for s in SIZES if a.min_bytes <= s <= a.max_bytes]:
        rcount = nbytes // 4 // n
        count = rcount * n
        rcounts = [rcount] * n
        x = torch.full((count,), float(rank + 1), dtype=torch.float32, device="cuda")
        x[::7] += 2.0
        total = torch.full((count,), float(n * (n + 1) // 2), dtype=torch.float32, device="cuda")
        total[::7] += 2.0 * n
        mine = total[rank * rcount:(rank + 1) * rcount].clone()
        for leg in legs:
            whole = leg in ("ar", "iar")
            y = torch.zeros(count if whole else rcount, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            if leg.startswith("irs") or leg == "iar":
                comm.barrier()
                comm.set("NB_ORDER", 1 if leg == "irs1" else 0)
                comm.barrier()
            call = {
                "rs": lambda: comm.reduce_scatter(x.data_ptr(), y.data_ptr(), rcounts, ty, op),
                "irs0": lambda: comm.ireduce_scatter(x.data_ptr(), y.data_ptr(), rcounts, ty, op).wait(),
                "irs1": lambda: comm.ireduce_scatter(x.data_ptr(), y.data_ptr(), rcounts, ty, op).wait(),
                "ar": lambda: comm.allreduce(x.data_ptr(), y.data_ptr(), count, ty, op),
                "iar": lambda: comm.iallreduce(x.data_ptr(), y.data_ptr(), count, ty, op).wait(),
            }[leg]
            warm = 5 if nbytes <= (16 << 20) else 3
            timed = a.iters if nbytes <= (16 << 20) else max(5, a.iters // 3)
            for _ in range(warm):
                call()
            ok = bool(torch.equal(y, total if whole else mine))
            samples = []
            for _ in range(timed):
                comm.barrier()
                t0 = time.perf_counter()
                call()
                samples.append(time.perf_counter() - t0)
            samples.sort()
            rows.append({"leg": leg + "_f32_sum", "label": a.label, "n": n, "bytes_per_rank": nbytes,
                         "algorithm": comm.last_algorithm(), "exact": ok, "calls": timed,
                         "median_us": round(statistics.median(samples) * 1e6, 1), "min_us": round(samples[0] * 1e6, 1),
                         "p90_us": round(samples[min(timed - 1, int(0.9 * timed))] * 1e6, 1)})
            del y
        del x, total, mine
        torch.cuda.empty_cache()
    comm.barrier()
    comm.destroy()
    bad = [r for r in rows if not r["exact"]]
    if rank == 0:
        for r in rows:
            print(json.dumps(r), flush=True)
    if bad:
        sys.exit(f"rank {rank}: wrong result at {[(r['leg'], r['bytes_per_rank']) for r in bad]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--min-bytes", type=int, default=SIZES[0])
    ap.add_argument("--max-bytes", type=int, default=SIZES[-1])
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--rank", type=int, default=-1)
    ap.add_argument("--key", default="")
    a = ap.parse_args()
    if a.rank >= 0:
        return rank_main(a)
    key = "irs" + uuid.uuid4().hex[:10]
    argv = [sys.executable, os.path.abspath(__file__), "--n", str(a.n), "--iters", str(a.iters), "--min-bytes",
            str(a.min_bytes), "--max-bytes", str(a.max_bytes), "--legs", a.legs, "--label", a.label, "--key", key]
    procs = [subprocess.Popen(argv + ["--rank", str(r)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(a.n)]
    outs, failed = [], False
    for p in procs:
        try:
            outs.append(p.communicate(timeout=300)[0])
        except subprocess.TimeoutExpired:
            p.kill()
            outs.append(p.communicate()[0])
            failed = True
    if failed or any(p.returncode for p in procs):
        sys.stderr.write("\n".join(outs))
        sys.exit(1)
    lines = [ln for ln in outs[0].splitlines() if ln.startswith("{")]
    if a.out:
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(ln + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
