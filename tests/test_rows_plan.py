"""The host side of the multi-segment row unpack (plan_rows_multi, ompi-release_amd/csrc/rt/ddt_rows_plan.hpp:
which pieces a launch keeps, the slot width they share, the blocks each one gets) against its contract
by brute force.  CPU only: tools/rows_plan_check.cpp compiles the header for the host alone; `make -C
tools check` runs the same program under AddressSanitizer + UBSan."""
import json
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rows_plan_matches_its_contract(tmp_path):
    exe = tmp_path / "rows_plan_check"
    subprocess.run(["g++", "-O2", "-Wall", "-Werror", "-o", str(exe), os.path.join(REPO, "tools", "rows_plan_check.cpp")],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["mismatches"] == 0 and res["checked"] > 100000
