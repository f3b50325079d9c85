"""MPI_Alltoall into a derived receive datatype, fused against unfused: a multi-process rehearsal (the
ranks are processes sharing ONE GPU, so no xGMI byte is timed -- every figure is a one-GPU figure).

Every rank receives `bytes_per_rank` bytes, bytes_per_rank / n from each peer, into
vector(blocks, 64, 128) of floats (256-byte runs every 512 bytes), one instance per peer:
  fused    mi355x_alltoallv_ddt: the peers' bytes are unpacked straight out of their memory, one launch;
  unfused  the sequence it replaces: mi355x_alltoallv into dense bytes, then mi355x_unpack per peer.
Both run in the same process, interleaved (fused, unfused, fused, ...), ten timed runs each after
warm-up, every run between two HIP events on the stream the calls use, after a barrier.  Rank 0's
medians and the unfused runs' spread (max - min) go to --out; both results are compared with each
other on the device at every size.

usage: python tools/move_ddt_bench.py [--n 4 8] [--out profiles/move_ddt.json]
       (starts the ranks itself; each rank is `python tools/move_ddt_bench.py --rank R --key K --n N`)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import uuid

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [64 << 10, 256 << 10, 1 << 20, 4 << 20, 16 << 20, 64 << 20, 256 << 20]
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
    rows = []
    for nbytes in [s for s in SIZES if a.min_bytes <= s <= a.max_bytes]:
        piece = nbytes // n // 256 * 256                # bytes from each peer: whole 256-byte runs
        blocks = piece // 256
        ddt = pkg.Ddt.vector(blocks, 64, 128, 4)
        ext = (ddt.extent + 255) // 256 * 256
        cnt, rdis = [1] * n, [q * ext for q in range(n)]
        sent, sdis = [piece] * n, [q * piece for q in range(n)]
        snd = torch.randint(0, 256, (piece * n,), dtype=torch.uint8, device="cuda")
        out_f = torch.zeros(ext * n, dtype=torch.uint8, device="cuda")
        out_u = torch.zeros(ext * n, dtype=torch.uint8, device="cuda")
        dense = torch.zeros(piece * n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def fused():
            comm.alltoallv_ddt(snd.data_ptr(), sent, sdis, out_f.data_ptr(), ddt, cnt, rdis)

        def unfused():
            comm.alltoallv(snd.data_ptr(), sent, sdis, dense.data_ptr(), sent, sdis)
            for q in range(n):
                ddt.unpack(1, out_u.data_ptr() + rdis[q], 0, dense.data_ptr() + sdis[q], piece)

        def timed(fn):
            comm.barrier()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3

        for _ in range(3):
            fused()
            unfused()
        torch.cuda.synchronize()
        same = bool(torch.equal(out_f, out_u)) and bool(out_f.any())
        tf, tu = [], []
        for _ in range(RUNS):
            tf.append(timed(fused))
            tu.append(timed(unfused))
        rows.append({"leg": "alltoall_into_vector_64_128_f32", "n": n, "ranks_share_one_gpu": True, "bytes_per_rank": nbytes,
                     "equal": same, "runs": RUNS, "fused_median_us": round(statistics.median(tf), 1),
                     "unfused_median_us": round(statistics.median(tu), 1), "unfused_spread_us": round(max(tu) - min(tu), 1),
                     "fused_min_us": round(min(tf), 1), "unfused_min_us": round(min(tu), 1)})
        del snd, out_f, out_u, dense
        torch.cuda.empty_cache()
    comm.barrier()
    comm.destroy()
    if rank == 0:
        for r in rows:
            print(json.dumps(r), flush=True)
    if not all(r["equal"] for r in rows):
        sys.exit(f"rank {rank}: fused and unfused results differ")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--min-bytes", type=int, default=SIZES[0])
    ap.add_argument("--max-bytes", type=int, default=SIZES[-1])
    ap.add_argument("--out", default="")
    ap.add_argument("--rank", type=int, default=-1)
    ap.add_argument("--key", default="")
    a = ap.parse_args()
    if a.rank >= 0:
        return rank_main(a)
    rows = []
    for n in a.n:
        key = "mvd" + uuid.uuid4().hex[:10]
        argv = [sys.executable, os.path.abspath(__file__), "--n", str(n), "--min-bytes", str(a.min_bytes), "--max-bytes",
                str(a.max_bytes), "--key", key]
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
            json.dump({"tool": "tools/move_ddt_bench.py", "note": "ranks are processes sharing one GPU: no xGMI byte is timed",
                       "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
