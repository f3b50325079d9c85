"""MPI_Scan through the engine at a sweep of message sizes: a multi-process rehearsal (the ranks are
processes sharing one GPU, so no xGMI byte is timed) of the chain flow against the partitioned flow.

fp32 SUM, not in place, 64 KiB .. 256 MiB per rank in powers of 4.  Per size: warm-up calls, then
timed calls one by one -- rank 0's wall time around the blocking call, which returns once every
rank's work has completed -- and their median, minimum and 90th percentile.  Inputs are small
integers, so every prefix is exact in fp32 and each size's result is checked on the device.

usage: python tools/scan_bench.py --n 4 [--part-min BYTES] [--label TEXT] [--out FILE]
       --part-min: SCAN_PART_MIN_BYTES for the run (1 = always partitioned, 0 = always the chain);
                   left out, the knob is not touched (the library's default; a build without the knob)
       (starts the ranks itself; each rank is `python tools/scan_bench.py --rank R --key K ...`)
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
SIZES = [64 << 10, 256 << 10, 1 << 20, 4 << 20, 16 << 20, 64 << 20, 256 << 20]


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
    if a.part_min is not None:
        comm.set("SCAN_PART_MIN_BYTES", a.part_min)
    op, ty = pkg.OP["SUM"], pkg.T["FLOAT"]
    rows = []
    for nbytes in [s for s in SIZES if a.min_bytes <= s <= a.max_bytes]:
        count = nbytes // 4
        x = torch.full((count,), float(rank + 1), dtype=torch.float32, device="cuda")
        x[::7] += 2.0
        y = torch.zeros_like(x)
        torch.cuda.synchronize()
        warm = 5 if nbytes <= (16 << 20) else 3
        timed = a.iters if nbytes <= (16 << 20) else max(5, a.iters // 3)
        for _ in range(warm):
            comm.scan(x.data_ptr(), y.data_ptr(), count, ty, op)
        want = torch.full((count,), float((rank + 1) * (rank + 2) // 2), dtype=torch.float32, device="cuda")
        want[::7] += 2.0 * (rank + 1)
        ok = bool(torch.equal(y, want))
        del want
        samples = []
        for _ in range(timed):
            comm.barrier()
            t0 = time.perf_counter()
            comm.scan(x.data_ptr(), y.data_ptr(), count, ty, op)
            samples.append(time.perf_counter() - t0)
        samples.sort()
        rows.append({"leg": "scan_f32_sum", "label": a.label, "n": n, "bytes_per_rank": nbytes,
                     "algorithm": comm.last_algorithm(), "exact": ok, "calls": timed,
                     "median_us": round(statistics.median(samples) * 1e6, 1), "min_us": round(samples[0] * 1e6, 1),
                     "p90_us": round(samples[min(timed - 1, int(0.9 * timed))] * 1e6, 1)})
        del x, y
        torch.cuda.empty_cache()
    comm.barrier()
    comm.destroy()
    bad = [r for r in rows if not r["exact"]]
    if rank == 0:
        for r in rows:
            print(json.dumps(r), flush=True)
    if bad:
        sys.exit(f"rank {rank}: wrong result at {[r['bytes_per_rank'] for r in bad]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--part-min", type=int, default=None)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--min-bytes", type=int, default=SIZES[0])
    ap.add_argument("--max-bytes", type=int, default=SIZES[-1])
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--rank", type=int, default=-1)
    ap.add_argument("--key", default="")
    a = ap.parse_args()
    if a.rank >= 0:
        return rank_main(a)
    key = "scan" + uuid.uuid4().hex[:10]
    argv = [sys.executable, os.path.abspath(__file__), "--n", str(a.n), "--iters", str(a.iters), "--min-bytes",
            str(a.min_bytes), "--max-bytes", str(a.max_bytes), "--label", a.label, "--key", key]
    if a.part_min is not None:
        argv += ["--part-min", str(a.part_min)]
    procs = [subprocess.Popen(argv + ["--rank", str(r)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(a.n)]
    outs, failed = [], False
    for p in procs:
        try:
            outs.append(p.communicate(timeout=420)[0])
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
