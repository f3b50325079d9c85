"""Row layouts of up to two levels, the host side of pulling through 3-D subarray layouts
(ompi-release_amd/csrc/rt/ddt_rows_plan.hpp): the normal form a layout's run tables are read in
(row_levels_view), the slot mapping with a second level on either end, the sender's rule and the plan of
the two-ended row gather with two-level ends, against their contracts by brute force.  CPU only:
tools/rows_levels_check.cpp compiles the header for the host alone; `make -C tools check` runs the same
program under AddressSanitizer + UBSan."""
import json
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rows_levels_plan_matches_its_contract(tmp_path):
    exe = tmp_path / "rows_levels_check"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-o", str(exe),
                    os.path.join(REPO, "tools", "rows_levels_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["mismatches"] == 0 and res["checked"] > 100000
