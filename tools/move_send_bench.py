"""MPI_Alltoall out of a derived send datatype, direct against packed: a multi-process rehearsal (the
ranks are processes sharing ONE GPU, so no xGMI byte is timed -- every figure is a one-GPU figure, and
what a strided read of short runs costs across a link cannot be seen here).  The measurement behind
the default of MOVE_SEND_MIN_RUN.

Every rank sends `bytes_per_rank` bytes (64 MiB), bytes_per_rank / n to each peer, out of a layout of
`run`-byte rows at stride 2 x run (1024 rows an instance), into dense bytes:
  direct   mi355x_alltoallv_ddt2 (MOVE_SEND_MIN_RUN = 1): the layout is published, nothing is packed,
           the peers gather the rows in one launch;
  packed   the sequence it replaces, still in the tree: mi355x_pack per peer into dense bytes, then
           mi355x_alltoallv.
Both run in the same process, interleaved (direct, packed, direct, ...), RUNS timed runs each after
warm-up, every run between two HIP events on the stream the calls use, after a barrier.  Rank 0's
medians, minima and each form's spread (max - min over its runs) go to --out; both results are
compared with each other on the device for every run length.

usage: python tools/move_send_bench.py [--n 2 4 8] [--out profiles/move_send.json]
       (starts the ranks itself; each rank is `python tools/move_send_bench.py --rank R --key K --n N`)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import uuid

HERE = os.path.dirname(os.path.abspath(__file__))
RUN_LENGTHS = [16, 64, 256, 4096]
ROWS = 1024          # rows an instance
RUNS = 10


def rank_main(a):
    import torch
    sys.path.insert(0, os.path.dirname(HERE))
    import bench
    pkg = bench.load_pkg()
    pkg.rt()
    rank, n = a.rank, a.n[0]
    torch.cuda.set_device(0)
    comm = pkg.Comm.create(a.key, rank, n, 0)
    comm.set("TIMEOUT_S", 120)
    comm.set("MOVE_SEND_MIN_RUN", 1)
    rows = []
    # every run length moves the same bytes: the buffers are allocated once (freeing and reallocating them per
    # leg hands the engine new allocations at addresses whose exports it has cached)
    total = a.bytes // n // (ROWS * max(RUN_LENGTHS)) * (ROWS * max(RUN_LENGTHS)) * n
    assert total, "--bytes holds no whole instance of the longest run per peer"
    # (bytes that differ from row to row)
    snd = (torch.arange(2 * total // 8, dtype=torch.int64, device="cuda") * 0x9E3779B97F4A7C15).view(torch.uint8)
    out_d = torch.zeros(total, dtype=torch.uint8, device="cuda")
    out_p = torch.zeros(total, dtype=torch.uint8, device="cuda")
    dense = torch.zeros(total, dtype=torch.uint8, device="cuda")
    for run in [r for r in RUN_LENGTHS if r in a.runs]:
        inst = ROWS * run                                  # packed bytes of an instance
        piece = total // n                                 # bytes to each peer
        per_peer = piece // inst                           # ... in instances
        ddt = pkg.Ddt.runs([0], [run], ROWS, 2 * run, 2 * inst)
        cnt, sdis = [per_peer] * n, [q * 2 * piece for q in range(n)]
        sent, ddis = [piece] * n, [q * piece for q in range(n)]
        out_d.zero_()
        out_p.zero_()
        torch.cuda.synchronize()
        assert comm.move_send_direct_ok(ddt, cnt)

        def direct():
            comm.alltoallv_ddt2(snd.data_ptr(), ddt, cnt, sdis, out_d.data_ptr(), None, sent, ddis)

        def packed():
            for q in range(n):
                ddt.pack(per_peer, snd.data_ptr() + sdis[q], 0, dense.data_ptr() + ddis[q], piece)
            comm.alltoallv(dense.data_ptr(), sent, ddis, out_p.data_ptr(), sent, ddis)

        def timed(fn):
            comm.barrier()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3

        before = comm.get("MOVE_SEND_DIRECT")
        for _ in range(3):
            direct()
            packed()
        torch.cuda.synchronize()
        assert comm.get("MOVE_SEND_DIRECT") == before + 3
        same = bool(torch.equal(out_d, out_p)) and bool(out_d.any())
        td, tp = [], []
        for _ in range(RUNS):
            td.append(timed(direct))
            tp.append(timed(packed))
        rows.append({"leg": "alltoall_out_of_rows_stride_2x", "n": n, "ranks_share_one_gpu": True, "bytes_per_rank": piece * n,
                     "run_bytes": run, "equal": same, "runs": RUNS, "direct_median_us": round(statistics.median(td), 1),
                     "packed_median_us": round(statistics.median(tp), 1), "direct_spread_us": round(max(td) - min(td), 1),
                     "packed_spread_us": round(max(tp) - min(tp), 1), "direct_min_us": round(min(td), 1),
                     "packed_min_us": round(min(tp), 1)})
    comm.barrier()
    comm.destroy()
    if rank == 0:
        for r in rows:
            print(json.dumps(r), flush=True)
    if not all(r["equal"] for r in rows):
        sys.exit(f"rank {rank}: the direct and the packed results differ")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--bytes", type=int, default=64 << 20)
    ap.add_argument("--runs", type=int, nargs="+", default=RUN_LENGTHS)
    ap.add_argument("--out", default="")
    ap.add_argument("--rank", type=int, default=-1)
    ap.add_argument("--key", default="")
    a = ap.parse_args()
    if a.rank >= 0:
        return rank_main(a)
    rows = []
    for n in a.n:
        key = "mvs" + uuid.uuid4().hex[:10]
        argv = [sys.executable, os.path.abspath(__file__), "--n", str(n), "--bytes", str(a.bytes), "--key", key, "--runs"] + \
               [str(r) for r in a.runs]
        procs = [subprocess.Popen(argv + ["--rank", str(r)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                 for r in range(n)]
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
        rows += [json.loads(ln) for ln in outs[0].splitlines() if ln.startswith("{")]
    for r in rows:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/move_send_bench.py", "note": "ranks are processes sharing one GPU: no xGMI byte is timed",
                       "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
