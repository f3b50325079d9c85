"""MPI_Alltoall of the z-pencils of a 3-D array, pulled through the two-level layout against the sequence
that replaces: a multi-process rehearsal (the ranks are processes sharing ONE GPU, so no xGMI byte is
timed -- every figure is a one-GPU figure, and what a strided read of short rows costs across a link
cannot be seen here).  The measurement behind the default of MOVE_ROW_LEVELS.

Every rank holds an nz x 65 x (n * sx + 1) array of floats or doubles and sends 64 MiB: to peer r the pencil
[0:nz, 0:64, r * sx:(r + 1) * sx] -- rows of `run` = sx elements (16, 64, 256, 4096 B), 64 rows a plane at
the array's row pitch, nz planes at its plane pitch, the type resized to one row so the pieces interleave in
the sender's memory.  The spare element of every array row makes the pitch a multiple of the element size
only, so floats move in 4-byte slots and doubles in 8-byte slots.  `send`: into dense bytes; `both`: into
the same pencils of the receiver's array.
  levels2  mi355x_alltoallv_ddt2 under MOVE_ROW_LEVELS = 2: the layout is published, nothing is packed, one
           launch gathers every peer's rows (into the receive layout too);
  levels1  the sequence under MOVE_ROW_LEVELS = 1, the one a caller makes when the rule says no: mi355x_pack
           per peer into dense bytes, then mi355x_alltoallv (`send`) or mi355x_alltoallv_ddt (`both`: the
           receive side unpacked peer by peer).
A tree whose engine has no MOVE_ROW_LEVELS knob (--tree: another build of the project, the parent commit as
the baseline) runs levels1 alone, which is all it has.  Forms run in the same process, interleaved, RUNS
timed runs each after warm-up, every run between two HIP events on the stream the calls use, after a
barrier; --rounds repeats the whole sweep, trees interleaved.  Rank 0's medians, minima and each form's
spread (max - min over its runs) go to --out.

usage: python tools/move_planes_bench.py [--n 2 4 8] [--tree . ../parent] [--rounds 2] [--out profiles/move_rows_levels.json]
       (starts the ranks itself; each rank is `python tools/move_planes_bench.py --rank R --key K --n N --tree T`)
"""
import argparse
import importlib.util
import json
import os
import statistics
import subprocess
import sys
import uuid

HERE = os.path.dirname(os.path.abspath(__file__))
RUN_LENGTHS = [16, 64, 256, 4096]
SY = 64              # rows a plane
RUNS = 10


def load_pkg(tree):
    spec = importlib.util.spec_from_file_location("ompi_release_amd", os.path.join(tree, "ompi-release_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["ompi_release_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def rank_main(a):
    import torch
    pkg = load_pkg(a.tree[0])
    pkg.rt()
    rank, n = a.rank, a.n[0]
    torch.cuda.set_device(0)
    comm = pkg.Comm.create(a.key, rank, n, 0)
    comm.set("TIMEOUT_S", 120)
    comm.set("MOVE_SEND_MIN_RUN", 1)
    has_levels = "MOVE_ROW_LEVELS" in pkg.KNOB
    rows = []
    piece = a.bytes // n                                       # bytes to each peer
    biggest = max((piece // (SY * run)) * (SY + 1) * (n * run + 8) for run in RUN_LENGTHS)
    # the buffers are allocated once (freeing and reallocating them per leg hands the engine new allocations at
    # addresses whose exports it has cached); bytes that differ from row to row
    snd = (torch.arange(biggest // 8 + 1, dtype=torch.int64, device="cuda") * 0x9E3779B97F4A7C15).view(torch.uint8)
    arr = [torch.zeros(biggest + 8, dtype=torch.uint8, device="cuda") for _ in range(2)]
    out = [torch.zeros(piece * n, dtype=torch.uint8, device="cuda") for _ in range(2)]
    dense = torch.zeros(piece * n, dtype=torch.uint8, device="cuda")
    for elem, ename in ((4, "float"), (8, "double")):
        for run in [r for r in RUN_LENGTHS if r in a.runs]:
            nz = piece // (SY * run)
            pitch = n * run + elem                              # one spare element a row
            plane = (SY + 1) * pitch                            # one spare row a plane
            assert nz >= 1 and nz * SY * run == piece
            ddt = pkg.Ddt.runs([j * pitch for j in range(SY)], [run] * SY, nz, plane, run)
            cnt, sdis = [1] * n, [q * run for q in range(n)]
            sent, ddis = [piece] * n, [q * piece for q in range(n)]
            for sides in ("send", "both"):
                both = sides == "both"
                res = arr if both else out
                for t in res:
                    t.zero_()
                torch.cuda.synchronize()

                def levels2():
                    comm.set("MOVE_ROW_LEVELS", 2)
                    comm.alltoallv_ddt2(snd.data_ptr(), ddt, cnt, sdis, res[0].data_ptr(), ddt if both else None,
                                        cnt if both else sent, sdis if both else ddis)

                def levels1():
                    if has_levels:
                        comm.set("MOVE_ROW_LEVELS", 1)
                    for q in range(n):
                        ddt.pack(1, snd.data_ptr() + sdis[q], 0, dense.data_ptr() + ddis[q], piece)
                    if both:
                        comm.alltoallv_ddt(dense.data_ptr(), sent, ddis, res[1].data_ptr(), ddt, cnt, sdis)
                    else:
                        comm.alltoallv(dense.data_ptr(), sent, ddis, res[1].data_ptr(), sent, ddis)

                def timed(fn):
                    comm.barrier()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    return e0.elapsed_time(e1) * 1e3

                forms = ([("levels2", levels2)] if has_levels else []) + [("levels1", levels1)]
                if has_levels:
                    comm.set("MOVE_ROW_LEVELS", 2)
                    assert comm.move_send_direct_ok(ddt, cnt)
                before = comm.get("MOVE_SEND_DIRECT")
                for _ in range(3):
                    for _, fn in forms:
                        fn()
                torch.cuda.synchronize()
                assert comm.get("MOVE_SEND_DIRECT") == before + (3 if has_levels else 0)
                same = bool(res[1].any()) and (not has_levels or bool(torch.equal(res[0], res[1])))
                ts = {name: [] for name, _ in forms}
                for _ in range(RUNS):
                    for name, fn in forms:
                        ts[name].append(timed(fn))
                row = {"leg": "alltoall_z_pencils", "sides": sides, "elem": ename, "n": n, "ranks_share_one_gpu": True,
                       "bytes_per_rank": piece * n, "run_bytes": run, "rows_per_plane": SY, "planes": nz, "equal": same, "runs": RUNS}
                for name, t in ts.items():
                    row.update({f"{name}_median_us": round(statistics.median(t), 1), f"{name}_min_us": round(min(t), 1),
                                f"{name}_spread_us": round(max(t) - min(t), 1)})
                rows.append(row)
    comm.barrier()
    comm.destroy()
    if rank == 0:
        for r in rows:
            print(json.dumps(r), flush=True)
    if not all(r["equal"] for r in rows):
        sys.exit(f"rank {rank}: the two forms' results differ")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--bytes", type=int, default=64 << 20)
    ap.add_argument("--runs", type=int, nargs="+", default=RUN_LENGTHS)
    ap.add_argument("--tree", nargs="+", default=[os.path.dirname(HERE)])
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--out", default="")
    ap.add_argument("--rank", type=int, default=-1)
    ap.add_argument("--key", default="")
    a = ap.parse_args()
    if a.rank >= 0:
        return rank_main(a)
    rows = []
    for rnd in range(a.rounds):
        for n in a.n:
            for tree in a.tree:
                key = "mvp" + uuid.uuid4().hex[:10]
                argv = [sys.executable, os.path.abspath(__file__), "--n", str(n), "--bytes", str(a.bytes), "--key", key,
                        "--tree", os.path.abspath(tree), "--runs"] + [str(r) for r in a.runs]
                procs = [subprocess.Popen(["timeout", "-k", "10", "300"] + argv + ["--rank", str(r)], stdout=subprocess.PIPE,
                                          stderr=subprocess.STDOUT, text=True) for r in range(n)]
                outs, failed = [], False
                for p in procs:
                    try:
                        outs.append(p.communicate(timeout=320)[0])
                    except subprocess.TimeoutExpired:
                        p.kill()
                        outs.append(p.communicate()[0])
                        failed = True
                if failed or any(p.returncode for p in procs):
                    sys.stderr.write("\n".join(outs))
                    sys.exit(1)
                for ln in outs[0].splitlines():
                    if ln.startswith("{"):
                        rows.append(dict(json.loads(ln), tree=os.path.relpath(tree, os.path.dirname(HERE)), round=rnd))
                        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/move_planes_bench.py", "note": "ranks are processes sharing one GPU: no xGMI byte is timed",
                       "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
