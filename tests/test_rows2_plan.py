"""The host side of pulling out of a send layout (ompi-release_amd/csrc/rt/ddt_rows_plan.hpp): the rule by
which a sender publishes its layout instead of packing (move_send_direct_ok), the plan of the two-ended
row gather (plan_rows2_multi: pieces kept, the slot width both ends share, the blocks each piece gets) and
the slot mapping the kernel applies on both ends, against their contracts by brute force.  CPU only:
tools/rows2_plan_check.cpp compiles the header for the host alone; `make -C tools check` runs the same
program under AddressSanitizer + UBSan."""
import json
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rows2_plan_matches_its_contract(tmp_path):
    exe = tmp_path / "rows2_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-o", str(exe),
                    os.path.join(REPO, "tools", "rows2_plan_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["mismatches"] == 0 and res["checked"] > 100000
